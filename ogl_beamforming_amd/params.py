"""ctypes mirrors of the parameter structures of include/ogl_beamformer_lib.h.

The reference ships the same structures to Python through a cffi-ready preprocessed
header (build.c:4798-4800) and to MATLAB through generated classes; field names, order
and sizes follow generated/beamformer.c:304-461 of the reference.
"""
import ctypes as C
import enum

MAX_CHANNELS = 256
MAX_EMISSIONS = 256
MAX_STAGES = 16
MAX_PARAMETER_BLOCKS = 16
FILTER_SLOTS = 4


class DataKind(enum.IntEnum):
    Int16 = 0
    Int16Complex = 1
    Float32 = 2
    Float32Complex = 3
    Float16 = 4
    Float16Complex = 5


DATA_KIND_BYTES = {0: 2, 1: 4, 2: 4, 3: 8, 4: 2, 5: 4}
DATA_KIND_NUMPY = {0: "int16", 1: "int16", 2: "float32", 3: "float32", 4: "float16", 5: "float16"}
DATA_KIND_COMPLEX = {0: False, 1: True, 2: False, 3: True, 4: False, 5: True}


class ShaderKind(enum.IntEnum):
    Decode = 0
    Filter = 1
    Demodulate = 2
    DAS = 3
    Hilbert = 4
    CoherencyWeighting = 5
    Reshape = 6
    MinMax = 7
    Sum = 8


class AcquisitionKind(enum.IntEnum):
    FORCES = 0
    UFORCES = 1
    HERCULES = 2
    RCA_VLS = 3
    RCA_TPW = 4
    UHERCULES = 5
    RACES = 6
    EPIC_FORCES = 7
    EPIC_UFORCES = 8
    EPIC_UHERCULES = 9
    Flash = 10
    HERO_PA = 11
    ULM = 12


class InterpolationMode(enum.IntEnum):
    Nearest = 0
    Linear = 1
    Cubic = 2


class RCAOrientation(enum.IntEnum):
    None_ = 0
    Rows = 1
    Columns = 2


class FilterKind(enum.IntEnum):
    Kaiser = 0
    MatchedChirp = 1


class LibError(enum.IntEnum):
    None_ = 0
    VersionMismatch = 1
    InvalidAccess = 2
    ParameterBlockOverflow = 3
    ParameterBlockUnallocated = 4
    ComputeStageOverflow = 5
    InvalidComputeStage = 6
    InvalidStartShader = 7
    InvalidDemodulationDataKind = 8
    InvalidImagePlane = 9
    InvalidFilterKind = 10
    InvalidDataKind = 11
    InvalidContrastMode = 12
    BufferOverflow = 13
    DataSizeMismatch = 14
    WorkQueueFull = 15
    ExportSpaceOverflow = 16
    SharedMemory = 17
    SyncVariable = 18
    FrameSizeOverflow = 19
    RFDataSizeOverflow = 20


class SineParameters(C.Structure):
    _fields_ = [("cycles", C.c_float), ("frequency", C.c_float)]


class ChirpParameters(C.Structure):
    _fields_ = [("duration", C.c_float), ("min_frequency", C.c_float), ("max_frequency", C.c_float)]


class _EmissionUnion(C.Union):
    _fields_ = [("sine", SineParameters), ("chirp", ChirpParameters)]


class EmissionParameters(C.Structure):
    _anonymous_ = ("u",)
    _fields_ = [("kind", C.c_int32), ("u", _EmissionUnion)]


class KaiserFilterParameters(C.Structure):
    _fields_ = [("cutoff_frequency", C.c_float), ("beta", C.c_float), ("length", C.c_uint32)]


class MatchedChirpFilterParameters(C.Structure):
    _fields_ = [("duration", C.c_float), ("min_frequency", C.c_float), ("max_frequency", C.c_float)]


class _FilterUnion(C.Union):
    _fields_ = [("kaiser", KaiserFilterParameters), ("matched_chirp", MatchedChirpFilterParameters)]


class FilterParameters(C.Structure):
    _anonymous_ = ("u",)
    _fields_ = [("kind", C.c_int32), ("sampling_frequency", C.c_float), ("complex", C.c_uint32),
                ("u", _FilterUnion)]


_PARAMETER_FIELDS = [
    ("das_voxel_transform", C.c_float * 16),
    ("xdc_transform", C.c_float * 16),
    ("xdc_element_pitch", C.c_float * 2),
    ("raw_data_dimensions", C.c_uint32 * 2),
    ("focal_vector", C.c_float * 2),
    ("transmit_receive_orientation", C.c_uint32),
    ("sample_count", C.c_uint32),
    ("channel_count", C.c_uint32),
    ("acquisition_count", C.c_uint32),
    ("acquisition_kind", C.c_int32),
    ("decode_mode", C.c_int32),
    ("sampling_mode", C.c_int32),
    ("time_offset", C.c_float),
    ("single_focus", C.c_uint32),
    ("single_orientation", C.c_uint32),
    ("output_points", C.c_int32 * 4),
    ("sampling_frequency", C.c_float),
    ("demodulation_frequency", C.c_float),
    ("speed_of_sound", C.c_float),
    ("f_number", C.c_float),
    ("interpolation_mode", C.c_int32),
    ("coherency_weighting", C.c_uint32),
    ("decimation_rate", C.c_uint32),
    ("contrast_mode", C.c_int32),
    ("emission_parameters", EmissionParameters),
    ("readi_group_count", C.c_uint32),
    ("readi_group", C.c_uint32),
]


class Parameters(C.Structure):
    _fields_ = list(_PARAMETER_FIELDS)


class SimpleParameters(C.Structure):
    _fields_ = list(_PARAMETER_FIELDS) + [
        ("channel_mapping", C.c_int16 * MAX_CHANNELS),
        ("sparse_elements", C.c_int16 * MAX_EMISSIONS),
        ("transmit_receive_orientations", C.c_uint8 * MAX_EMISSIONS),
        ("steering_angles", C.c_float * MAX_EMISSIONS),
        ("focal_depths", C.c_float * MAX_EMISSIONS),
        ("compute_stages", C.c_int32 * MAX_STAGES),
        ("compute_stage_parameters", C.c_int32 * MAX_STAGES),
        ("compute_stages_count", C.c_uint32),
        ("data_kind", C.c_int32),
    ]


class LiveImagingParameters(C.Structure):
    _fields_ = [
        ("active", C.c_uint32), ("save_enabled", C.c_uint32), ("save_active", C.c_uint32),
        ("acquisition_kind", C.c_uint32), ("acquisition_kind_enabled_flags", C.c_uint64),
        ("transmit_power", C.c_float), ("image_plane_offsets", C.c_float * 4),
        ("tgc_control_points", C.c_float * 8), ("save_name_tag_length", C.c_int32),
        ("save_name_tag", C.c_uint8 * 128),
    ]


class ComputeStatsTable(C.Structure):
    _fields_ = [
        ("shader_count", C.c_uint64), ("shader_ids", C.c_uint32 * MAX_STAGES),
        ("times", (C.c_float * MAX_STAGES) * 32), ("rf_time_deltas", C.c_float * 32),
    ]


HIP_MAX_TIMED_STAGES = 24


class HipFrameInfo(C.Structure):
    _fields_ = [("device_pointer", C.c_void_p), ("size_bytes", C.c_uint64), ("points", C.c_uint32 * 3),
                ("data_kind", C.c_uint32), ("frame_id", C.c_uint32), ("parameter_block", C.c_uint32)]


class HipFrameTimings(C.Structure):
    _fields_ = [
        ("stage_count", C.c_uint32), ("stage_kind", C.c_uint32 * HIP_MAX_TIMED_STAGES),
        ("stage_ms", C.c_float * HIP_MAX_TIMED_STAGES), ("frame_ms", C.c_float),
        ("das_pairs", C.c_uint64), ("das_voxels", C.c_uint64), ("das_taps", C.c_uint32),
        ("das_sample_bytes", C.c_uint32), ("das_path", C.c_uint32), ("staged_window_violations", C.c_uint32),
        ("tile_staged_chunks", C.c_uint32), ("tile_gather_chunks", C.c_uint32), ("das_row_end_planes", C.c_uint32),
    ]


class HipBurstDescription(C.Structure):
    _fields_ = [("burst_kernel", C.c_uint32), ("single_path", C.c_int32), ("frames_per_thread", C.c_uint32),
                ("das_launches", C.c_uint32), ("stage_launches", C.c_uint32), ("min_frames", C.c_uint32), ("reason", C.c_char * 160)]


class HipBurstInfo(C.Structure):
    _fields_ = [("route", HipBurstDescription), ("first_frame_id", C.c_uint32), ("frame_count", C.c_uint32), ("stage_count", C.c_uint32),
                ("stage_kind", C.c_uint32 * HIP_MAX_TIMED_STAGES), ("stage_ms", C.c_float * HIP_MAX_TIMED_STAGES), ("burst_ms", C.c_float)]


class HipReadiImageDescription(C.Structure):
    _fields_ = [("transmit_count", C.c_uint32), ("das_path", C.c_int32), ("das_launches", C.c_uint32), ("stage_launches", C.c_uint32),
                ("decode_launches", C.c_uint32), ("reason", C.c_char * 160)]


class HipReadiImageInfo(C.Structure):
    _fields_ = [("route", HipReadiImageDescription), ("frame_id", C.c_uint32), ("rf_frame_count", C.c_uint32), ("stage_count", C.c_uint32),
                ("stage_kind", C.c_uint32 * HIP_MAX_TIMED_STAGES), ("stage_ms", C.c_float * HIP_MAX_TIMED_STAGES), ("image_ms", C.c_float)]


HIP_MAX_BURST_FRAMES = 1024
HIP_DAS_PATH_NO_BURST_KERNEL = 0x400     # beamformer_hip_set_das_path flag: bursts run the single-frame DAS kernel once per frame


HIP_MAX_VIEWS = 1024
HIP_DAS_PATH_NO_VIEWS_KERNEL = 0x800      # beamformer_hip_set_das_path flag: a views push runs every view's single-frame DAS kernel
HIP_DAS_PATH_PREFER_VIEWS_KERNEL = 0x1000 # ... flag: the views kernel takes the eligible views however few their tiles
HIP_DAS_PATH_FAIL_VIEWS_DAS = 0x2000      # ... flag: a views push fails at its DAS stage, after its ids are taken (tombstones, for tests)


class HipView(C.Structure):
    """BeamformerHipView: one grid of a views push"""
    _fields_ = [("das_voxel_transform", C.c_float * 16), ("output_points", C.c_uint32 * 3), ("image_plane_tag", C.c_uint32)]


class HipViewsDescription(C.Structure):
    _fields_ = [("kernel_views", C.c_uint32), ("das_launches", C.c_uint32), ("min_tiles", C.c_uint32),
                ("path", C.c_int8 * HIP_MAX_VIEWS), ("reason", C.c_char * 160)]


class HipViewsInfo(C.Structure):
    _fields_ = [("route", HipViewsDescription), ("first_frame_id", C.c_uint32), ("view_count", C.c_uint32), ("stage_count", C.c_uint32),
                ("stage_kind", C.c_uint32 * HIP_MAX_TIMED_STAGES), ("stage_ms", C.c_float * HIP_MAX_TIMED_STAGES), ("views_ms", C.c_float),
                ("decide_us", C.c_float)]


class HipBurstViewsDescription(C.Structure):
    _fields_ = [("rung", C.c_uint32), ("kernel_views", C.c_uint32), ("frame_kernel_views", C.c_uint32), ("das_launches", C.c_uint32),
                ("stage_launches", C.c_uint32), ("frames_per_thread", C.c_uint32), ("min_frames", C.c_uint32),
                ("path", C.c_int8 * HIP_MAX_VIEWS), ("reason", C.c_char * 160)]


class HipBurstViewsInfo(C.Structure):
    _fields_ = [("route", HipBurstViewsDescription), ("first_frame_id", C.c_uint32), ("frame_count", C.c_uint32), ("view_count", C.c_uint32),
                ("stage_count", C.c_uint32), ("stage_kind", C.c_uint32 * HIP_MAX_TIMED_STAGES), ("stage_ms", C.c_float * HIP_MAX_TIMED_STAGES),
                ("push_ms", C.c_float), ("decide_us", C.c_float)]


HIP_MAX_VARIANTS = 64
HIP_DAS_PATH_NO_VARIANTS_KERNEL = 0x4000      # beamformer_hip_set_das_path flag: a variants push runs every variant's single-frame DAS kernel
HIP_DAS_PATH_PREFER_VARIANTS_KERNEL = 0x8000  # ... flag: the variants kernel takes the eligible variants however few their tiles
HIP_DAS_PATH_WARP_DIRECT = 0x10000            # ... flag: every tile of beamformer_hip_warp_last_frames takes the direct path (same bytes)


class HipDasVariant(C.Structure):
    """BeamformerHipDasVariant: one candidate of a variants push"""
    _fields_ = [("speed_of_sound", C.c_float), ("time_offset", C.c_float), ("f_number", C.c_float)]


class HipVariantsDescription(C.Structure):
    _fields_ = [("kernel_variants", C.c_uint32), ("fused_launches", C.c_uint32), ("das_launches", C.c_uint32), ("kernel_tiles", C.c_uint32),
                ("min_tiles", C.c_uint32), ("min_variants", C.c_uint32), ("path", C.c_int8 * HIP_MAX_VARIANTS), ("taken", C.c_uint8 * HIP_MAX_VARIANTS),
                ("reason", C.c_char * 160)]


class HipVariantsInfo(C.Structure):
    _fields_ = [("route", HipVariantsDescription), ("first_frame_id", C.c_uint32), ("variant_count", C.c_uint32), ("stage_count", C.c_uint32),
                ("stage_kind", C.c_uint32 * HIP_MAX_TIMED_STAGES), ("stage_ms", C.c_float * HIP_MAX_TIMED_STAGES), ("variants_ms", C.c_float),
                ("decide_us", C.c_float)]


HIP_MAX_SCORED_FRAMES = 1024


class HipFrameRegion(C.Structure):
    """BeamformerHipFrameRegion: a box of voxel indices, x, y, z"""
    _fields_ = [("first", C.c_uint32 * 3), ("count", C.c_uint32 * 3)]


class HipFrameMetrics(C.Structure):
    """BeamformerHipFrameMetrics: one frame's row of beamformer_hip_score_last_frames (no padding: rows compare byte for byte)"""
    _fields_ = [("frame_id", C.c_uint32), ("parameter_block", C.c_uint32), ("data_kind", C.c_uint32), ("image_plane_tag", C.c_uint32),
                ("points", C.c_uint32 * 3), ("region_first", C.c_uint32 * 3), ("region_count", C.c_uint32 * 3), ("max_index", C.c_uint32 * 3),
                ("voxels", C.c_uint64), ("non_finite", C.c_uint64), ("gradient_pairs", C.c_uint64 * 3),
                ("sum_abs", C.c_double), ("sum_abs2", C.c_double), ("sum_abs4", C.c_double), ("gradient2", C.c_double * 3),
                ("max_abs", C.c_float), ("reserved", C.c_uint32)]


HIP_MAX_PEAKS_PER_FRAME = 65536


class HipFramePeak(C.Structure):
    """BeamformerHipFramePeak: one local maximum of beamformer_hip_find_peaks_last_frames (32 bytes, no padding)"""
    _fields_ = [("index", C.c_uint32 * 3), ("magnitude", C.c_float), ("offset", C.c_float * 3), ("fitted", C.c_uint32)]


class HipFramePeaks(C.Structure):
    """BeamformerHipFramePeaks: one frame's row of beamformer_hip_find_peaks_last_frames (80 bytes, no padding)"""
    _fields_ = [("frame_id", C.c_uint32), ("parameter_block", C.c_uint32), ("data_kind", C.c_uint32), ("image_plane_tag", C.c_uint32),
                ("points", C.c_uint32 * 3), ("region_first", C.c_uint32 * 3), ("region_count", C.c_uint32 * 3),
                ("threshold", C.c_float), ("first", C.c_uint32), ("stored", C.c_uint32), ("found", C.c_uint64), ("above_threshold", C.c_uint64)]


HIP_MAX_QUANTILES = 16          # BEAMFORMER_HIP_MAX_QUANTILES
HIP_QUANTILE_BINS = 2048        # BEAMFORMER_HIP_QUANTILE_BINS


class HipFrameQuantile(C.Structure):
    """BeamformerHipFrameQuantile: one order statistic of beamformer_hip_quantiles_last_frames (48 bytes, no padding)"""
    _fields_ = [("fraction", C.c_double), ("rank", C.c_uint64), ("below", C.c_uint64), ("equal", C.c_uint64),
                ("value", C.c_float), ("magnitude", C.c_float), ("threshold", C.c_float), ("reserved", C.c_uint32)]


class HipFrameQuantiles(C.Structure):
    """BeamformerHipFrameQuantiles: one frame's row of beamformer_hip_quantiles_last_frames (80 bytes, no padding)"""
    _fields_ = [("frame_id", C.c_uint32), ("parameter_block", C.c_uint32), ("data_kind", C.c_uint32), ("image_plane_tag", C.c_uint32),
                ("points", C.c_uint32 * 3), ("region_first", C.c_uint32 * 3), ("region_count", C.c_uint32 * 3),
                ("first", C.c_uint32), ("stored", C.c_uint32), ("reserved", C.c_uint32), ("voxels", C.c_uint64), ("non_finite", C.c_uint64)]


HIP_MAX_MAP_VOXELS = 1 << 28    # BEAMFORMER_HIP_MAX_MAP_VOXELS


class HipMapDeposits(C.Structure):
    """BeamformerHipMapDeposits: one frame's row of beamformer_hip_accumulate_peaks_last_frames (96 bytes, no padding)"""
    _fields_ = [("frame_id", C.c_uint32), ("parameter_block", C.c_uint32), ("data_kind", C.c_uint32), ("image_plane_tag", C.c_uint32),
                ("points", C.c_uint32 * 3), ("region_first", C.c_uint32 * 3), ("region_count", C.c_uint32 * 3),
                ("threshold", C.c_float), ("reserved", C.c_uint32 * 2), ("found", C.c_uint64), ("above_threshold", C.c_uint64),
                ("deposited", C.c_uint64), ("outside", C.c_uint64)]


class HipMapInfo(C.Structure):
    """BeamformerHipMapInfo: the localisation map's grid and its totals since the reset (32 bytes, no padding)"""
    _fields_ = [("points", C.c_uint32 * 3), ("calls", C.c_uint32), ("deposited", C.c_uint64), ("outside", C.c_uint64)]


HIP_MAX_TRACK_MAP_VOXELS = 1 << 26     # BEAMFORMER_HIP_MAX_TRACK_MAP_VOXELS
HIP_MAX_PAIR_DISTANCE = 1048576.0      # BEAMFORMER_HIP_MAX_PAIR_DISTANCE
HIP_TRACK_MAP_COMPONENTS = 5           # BEAMFORMER_HIP_TRACK_MAP_COMPONENTS


class HipPeakPair(C.Structure):
    """BeamformerHipPeakPair: one link of beamformer_hip_pair_peaks_last_frames (48 bytes, no padding)"""
    _fields_ = [("frame", C.c_uint32), ("a", C.c_uint32), ("b", C.c_uint32), ("deposited", C.c_uint32),
                ("displacement", C.c_double * 3), ("distance2", C.c_double)]


class HipPeakPairs(C.Structure):
    """BeamformerHipPeakPairs: one frame pair's row of beamformer_hip_pair_peaks_last_frames (72 bytes, no padding)"""
    _fields_ = [("frame_id", C.c_uint32 * 2), ("threshold", C.c_float * 2), ("peaks", C.c_uint32 * 2), ("unplaced", C.c_uint32 * 2),
                ("unpaired", C.c_uint32 * 2), ("first", C.c_uint32), ("pairs", C.c_uint32), ("deposited", C.c_uint32), ("outside", C.c_uint32),
                ("found", C.c_uint64 * 2)]


class HipTrackMapInfo(C.Structure):
    """BeamformerHipTrackMapInfo: the track map's grid and its totals since the reset (40 bytes, no padding)"""
    _fields_ = [("points", C.c_uint32 * 3), ("calls", C.c_uint32), ("pairs", C.c_uint64), ("deposited", C.c_uint64), ("outside", C.c_uint64)]


HIP_TRACK_DEPOSIT_POINTS = 1           # BEAMFORMER_HIP_TRACK_DEPOSIT_POINTS
HIP_TRACK_DEPOSIT_LINKS = 2            # BEAMFORMER_HIP_TRACK_DEPOSIT_LINKS


class HipPeakTrack(C.Structure):
    """BeamformerHipPeakTrack: one kept track of beamformer_hip_track_peaks_last_frames (48 bytes, no padding)"""
    _fields_ = [("frame", C.c_uint32), ("rank", C.c_uint32), ("length", C.c_uint32), ("first", C.c_uint32), ("flags", C.c_uint32),
                ("reserved", C.c_uint32), ("displacement", C.c_double * 3)]


class HipTrackPoint(C.Structure):
    """BeamformerHipTrackPoint: one peak of a kept track of beamformer_hip_track_peaks_last_frames (40 bytes, no padding)"""
    _fields_ = [("track", C.c_uint32), ("frame", C.c_uint32), ("rank", C.c_uint32), ("deposited", C.c_uint32), ("position", C.c_double * 3)]


class HipTrackedFrame(C.Structure):
    """BeamformerHipTrackedFrame: one frame's row of beamformer_hip_track_peaks_last_frames (56 bytes, no padding)"""
    _fields_ = [("frame_id", C.c_uint32), ("threshold", C.c_float), ("peaks", C.c_uint32), ("unplaced", C.c_uint32), ("heads", C.c_uint32),
                ("kept_heads", C.c_uint32), ("kept_points", C.c_uint32), ("kept_links", C.c_uint32), ("points_deposited", C.c_uint32),
                ("points_outside", C.c_uint32), ("links_deposited", C.c_uint32), ("links_outside", C.c_uint32), ("found", C.c_uint64)]


assert C.sizeof(HipPeakTrack) == 48 and C.sizeof(HipTrackPoint) == 40 and C.sizeof(HipTrackedFrame) == 56

HIP_MAX_TRACK_SMOOTH = 8               # BEAMFORMER_HIP_MAX_TRACK_SMOOTH
HIP_MAX_LINK_SAMPLES = 4096.0          # BEAMFORMER_HIP_MAX_LINK_SAMPLES


class HipDrawnFrame(C.Structure):
    """BeamformerHipDrawnFrame: one frame's row of beamformer_hip_draw_tracks_last_frames (64 bytes, no padding)"""
    _fields_ = [("frame_id", C.c_uint32), ("threshold", C.c_float), ("peaks", C.c_uint32), ("unplaced", C.c_uint32), ("kept_points", C.c_uint32),
                ("kept_links", C.c_uint32), ("lone", C.c_uint32), ("links_skipped", C.c_uint32), ("samples", C.c_uint32), ("repeats", C.c_uint32),
                ("points_deposited", C.c_uint32), ("points_outside", C.c_uint32), ("links_deposited", C.c_uint32), ("links_outside", C.c_uint32),
                ("found", C.c_uint64)]


assert C.sizeof(HipDrawnFrame) == 64

HIP_MAX_ENSEMBLE_FRAMES = 256
HIP_MAX_GRAM_BOXES = 1024               # BEAMFORMER_HIP_MAX_GRAM_BOXES
HIP_MAX_GRAM_BOX_ENTRIES = 1 << 22      # BEAMFORMER_HIP_MAX_GRAM_BOX_ENTRIES: boxes x count x count
HIP_MAX_MIX_NODES = 1024                # BEAMFORMER_HIP_MAX_MIX_NODES: product of nodes
HIP_MAX_MIX_FIELD_ENTRIES = 1 << 22     # BEAMFORMER_HIP_MAX_MIX_FIELD_ENTRIES: product of nodes x out_count x count
HIP_MAX_LAGS = 4                # BEAMFORMER_HIP_MAX_LAGS
HIP_MAX_SPATIAL_TAPS = 33       # BEAMFORMER_HIP_MAX_SPATIAL_TAPS


class HipSpatialMode(enum.IntEnum):
    """BeamformerHipSpatialMode (beamformer_hip_convolve_last_frames)"""
    Zero = 0
    Normalised = 1


class HipEnsembleInfo(C.Structure):
    """BeamformerHipEnsembleInfo: what beamformer_hip_gram_last_frames reduced (64 bytes, no padding)"""
    _fields_ = [("count", C.c_uint32), ("data_kind", C.c_uint32), ("points", C.c_uint32 * 3), ("region_first", C.c_uint32 * 3),
                ("region_count", C.c_uint32 * 3), ("first_frame_id", C.c_uint32), ("voxels", C.c_uint64), ("non_finite", C.c_uint64)]


HIP_MAX_SHIFT = 16                      # BEAMFORMER_HIP_MAX_SHIFT
HIP_MAX_SHIFTS = 1089                   # BEAMFORMER_HIP_MAX_SHIFTS
HIP_MAX_CORRELATION_REGIONS = 256       # BEAMFORMER_HIP_MAX_CORRELATION_REGIONS
HIP_MAX_CORRELATION_ENTRIES = 1 << 20   # BEAMFORMER_HIP_MAX_CORRELATION_ENTRIES


class HipShiftCorrelation(C.Structure):
    """BeamformerHipShiftCorrelation: one entry (region, frame, shift) of beamformer_hip_correlate_last_frames (40 bytes, no padding)"""
    _fields_ = [("re", C.c_double), ("im", C.c_double), ("energy_reference", C.c_double), ("energy_frame", C.c_double), ("terms", C.c_uint64)]


class HipCorrelationInfo(C.Structure):
    """BeamformerHipCorrelationInfo: what beamformer_hip_correlate_last_frames reduced (56 bytes, no padding)"""
    _fields_ = [("count", C.c_uint32), ("reference", C.c_uint32), ("data_kind", C.c_uint32), ("region_count", C.c_uint32),
                ("points", C.c_uint32 * 3), ("max_shift", C.c_uint32 * 3), ("shifts", C.c_uint32),
                ("first_frame_id", C.c_uint32), ("reference_frame_id", C.c_uint32), ("reserved", C.c_uint32)]


class HipDisplacement(C.Structure):
    """BeamformerHipDisplacement: one table's row of beamformer_hip_displacements_from_correlation (40 bytes, no padding)"""
    _fields_ = [("displacement", C.c_float * 3), ("shift", C.c_int32 * 3), ("coefficient", C.c_float), ("phase", C.c_float),
                ("fitted", C.c_uint32), ("at_window_edge", C.c_uint32)]


HIP_MAX_WARP_NODES = 4096               # BEAMFORMER_HIP_MAX_WARP_NODES
HIP_MAX_WARP_ENTRIES = 32768            # BEAMFORMER_HIP_MAX_WARP_ENTRIES
HIP_MAX_WARP_DISPLACEMENT = 65536.0     # BEAMFORMER_HIP_MAX_WARP_DISPLACEMENT


class HipWarpInterpolation(enum.IntEnum):
    """BeamformerHipWarpInterpolation (beamformer_hip_warp_last_frames)"""
    Linear = 0
    Cubic = 1


class HipWarpEdge(enum.IntEnum):
    """BeamformerHipWarpEdge (beamformer_hip_warp_last_frames)"""
    Zero = 0
    Clamp = 1


class FrameScore(enum.IntEnum):
    """BeamformerHipFrameScore: the criteria of beamformer_hip_rank_frames"""
    Energy = 0
    MeanMagnitude = 1
    Sharpness = 2
    GradientEnergy = 3


class DasPath(enum.IntEnum):
    """BeamformerHipFrameTimings::das_path / BeamformerHipDasDescription::path (csrc/das_select.h)"""
    General = 0
    Gather = 1
    Staged = 2
    Factored = 3
    Hercules = 4
    Tile = 5


class HipDeviceInfo(C.Structure):
    _fields_ = [("ordinal", C.c_int32), ("peer_access", C.c_int32), ("slab_first", C.c_uint32), ("slab_count", C.c_uint32),
                ("peer_copy_ms", C.c_float), ("das_ms", C.c_float), ("frame_ms", C.c_float),
                ("rf_checksum", C.c_uint64), ("rf_bytes", C.c_uint64)]


class HipDasDescription(C.Structure):
    _fields_ = [("path", C.c_int32), ("kernel", C.c_char * 48), ("name", C.c_char * 64), ("declined", (C.c_char * 160) * 8),
                ("tile_shift", C.c_uint32 * 3), ("blocks", C.c_uint32 * 3), ("split_shift", C.c_uint32), ("tile_walk", C.c_uint32),
                ("row_end_planes", C.c_uint32), ("tile_window_samples", C.c_uint32), ("u_axis", C.c_uint32), ("u_shift", C.c_uint32), ("v_shift", C.c_uint32), ("window_samples", C.c_uint32),
                ("uniform_tables", C.c_uint32), ("lds_bytes", C.c_uint32), ("threads", C.c_uint32), ("channel_chunk", C.c_uint32),
                ("hercules_prepared_copy", C.c_uint32), ("tile_spread_estimate", C.c_float), ("tile_estimate_shift", C.c_uint32 * 3), ("row_ends", C.c_uint32),
                ("row_end_path", C.c_int32)]


class HipPlanStage(C.Structure):
    _fields_ = [("kind", C.c_int32), ("in_kind", C.c_int32), ("out_kind", C.c_int32),
                ("in_stride", C.c_int64 * 3), ("out_stride", C.c_int64 * 3)]


class HipPlan(C.Structure):
    _fields_ = [("stage_count", C.c_uint32), ("stages", HipPlanStage * MAX_STAGES),
                ("das_samples", C.c_uint32), ("iq_pipeline", C.c_uint32),
                ("das_sampling_frequency", C.c_float), ("das_time_offset", C.c_float),
                ("das_voxel_transform", C.c_float * 16), ("intermediate_bytes", C.c_uint64)]


class UploadRoute(enum.IntEnum):
    PinnedInPlace = 0
    CopyEngineDirect = 1
    CopyEngineStaged = 2
    DeviceBorrowed = 3
    DeviceCopy = 4
    DeviceIngest = 5


class HipUploadDescription(C.Structure):
    _fields_ = [("route", C.c_uint32), ("ingest_kernel", C.c_uint32), ("copy_bytes", C.c_uint32), ("a1s2_base", C.c_uint32),
                ("rf_bytes", C.c_uint64), ("upload_bytes", C.c_uint64), ("name", C.c_char * 32)]


class HipZbpPayload(C.Structure):
    _fields_ = [("major", C.c_uint32), ("data_kind", C.c_uint32), ("compression_kind", C.c_uint32),
                ("reserved", C.c_uint32), ("offset", C.c_uint64), ("size", C.c_uint64)]


assert C.sizeof(Parameters) == 264
assert C.sizeof(SimpleParameters) == 3728
assert C.sizeof(FilterParameters) == 24
assert C.sizeof(LiveImagingParameters) == 208
assert C.sizeof(ComputeStatsTable) == 2248
