"""The RF ingest matrix (tests/test_ingest_host.py on the CPU, tests/test_gpu_ingest.py on the device): every upload route of
csrc/executor.cpp's decide_upload, every lane width of ingest_copy_kernel with a non-identity mapping, every instantiation of
ingest_a1s2_kernel, and both kernels' grid-stride loops past their first trip.

Every case is {Decode (decode_mode None), DAS} on a 16 x 1 x 16 grid with noise RF and a fixed seed: the planner drops the Decode, so
the DAS input is the ingested RF through at most an exact conversion (int16 / binary16 -> binary32) and is judged by its bits.

A case's NAME promises its route (group + size), its kernel and its lane width; Case holds the promise in fields, the host test asks
beamformer_hip_describe_upload whether the library keeps it.

The module's own references, independent of oracle/:
  mapped_rf    the RF slot after ingest: rows picked by the channel mapping, raw padding dropped; for A1S2 a - b - c in the data
               kind's scalar type, one rounding per operation, on the first sample_count x element_count scalars, the rest of the
               row zero (lib/ogl_beamformer_lib.c:478-487, :553 of the reference);
  rf_checksum  its position-weighted checksum as rf_checksum_kernel forms it: 8-byte words, sum w[i] (i + 1) mod 2^64, a tail under
               8 bytes ignored."""
import dataclasses
import functools

import numpy as np

from ogl_beamforming_amd import configs as cfg
from ogl_beamforming_amd import params as P

S = P.ShaderKind
DK = P.DataKind
R = P.UploadRoute
FS, FD, PITCH = 25e6, 6.25e6, 0.3e-3
GRID = (16, 1, 16)
BASE_OF = {"int16": 0, "float32": 1, "float16": 2}          # bf_kernels.h BF_BASE_*
COPY_TRIP = 4096 * 256                                      # elements one trip of a grid-stride loop covers: the grid is clamped at 4096 blocks of 256


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    group: str                  # small, large, long, planted
    kind: DK
    channels: int
    transmits: int
    samples: int
    pad: int = 0
    contrast: bool = False
    mapping: str = "shuffled"   # shuffled, identity, swapped
    seed: int = 0
    route: R = R.PinnedInPlace  # host push
    kernel: int = 1             # 0 none, 1 copy, 2 A1S2
    width: int = 0              # copy kernel: bytes per lane
    device_route: R = R.DeviceIngest


def _small(kind, pad, width, seed, **kw):
    contrast = kw.get("contrast", False)
    name = f"{kind.name}_{'a1s2' if contrast else f'w{width}'}_pad{pad}"
    return Case(name, "small", kind, 8, 2, 256, pad=pad, seed=seed, kernel=2 if contrast else 1, width=0 if contrast else width, **kw)


# ---- small (under the copy-engine threshold): six data kinds x contrast off / on, shuffled.  Row bytes = scalar bytes x
# (512 samples + pad): Int16 552 x 2 = 16 x 69, 514 x 2 = 4 x 257, 549 x 2 = 2 x 549; Int16Complex 515 x 4 = 4 x 515; Float32 516 x 4 =
# 16 x 129; Float32Complex 513 x 8 = 4 x 1026 (an odd element count); Float16 517 x 2 = 2 x 517; Float16Complex 516 x 4 = 16 x 129
_CASES = [
    _small(DK.Int16, 40, 16, 1), _small(DK.Int16, 2, 4, 2), _small(DK.Int16, 37, 2, 3),
    _small(DK.Int16Complex, 3, 4, 4), _small(DK.Float32, 4, 16, 5), _small(DK.Float32Complex, 1, 4, 6),
    _small(DK.Float16, 5, 2, 7), _small(DK.Float16Complex, 4, 16, 8),
    _small(DK.Int16, 37, 0, 11, contrast=True), _small(DK.Int16Complex, 3, 0, 12, contrast=True),
    _small(DK.Float32, 0, 0, 13, contrast=True), _small(DK.Float32Complex, 1, 0, 14, contrast=True),
    _small(DK.Float16, 5, 0, 15, contrast=True), _small(DK.Float16Complex, 2, 0, 16, contrast=True),
    # 171 samples x 3 transmits = 513: the MAPPED row is 1026 bytes, 2 mod 4
    Case("Int16_w2_odd_row", "small", DK.Int16, 8, 3, 171, seed=21, width=2),
    # identity mapping, padding only: not direct (the rows have to be repacked)
    Case("Int16_w16_identity_pad8", "small", DK.Int16, 8, 2, 256, pad=8, mapping="identity", seed=22, width=16),
    # identity mapping, no padding: the mapped layout.  Int16 plans start with the converting Reshape, which borrows a device buffer;
    # Float32 plans start with DAS, which gets a device-to-device copy
    Case("Int16_w16_identity", "small", DK.Int16, 8, 2, 256, mapping="identity", seed=23, width=16, device_route=R.DeviceBorrowed),
    Case("Float32_w16_identity", "small", DK.Float32, 8, 2, 256, mapping="identity", seed=24, width=16, device_route=R.DeviceCopy),
    # ---- large (at or over the threshold).  64 x 17 x 4096 Int16: 8.5 MiB; big_f32c_shuffled is 8 MiB to the byte
    Case("big_direct", "large", DK.Int16, 64, 17, 4096, mapping="identity", seed=31, route=R.CopyEngineDirect, kernel=0, device_route=R.DeviceBorrowed),
    Case("big_shuffled_padded", "large", DK.Int16, 64, 17, 4096, pad=40, seed=32, route=R.CopyEngineStaged, width=16),
    Case("big_a1s2", "large", DK.Int16, 64, 6, 4096, contrast=True, seed=33, route=R.CopyEngineStaged, kernel=2),
    Case("big_f32c_shuffled", "large", DK.Float32Complex, 64, 4, 4096, seed=34, route=R.CopyEngineStaged, width=16),
    # ---- long rows: more than 4096 x 256 elements of the kernel's lane width per row
    Case("long_i16_w2", "long", DK.Int16, 2, 1, 1050000, pad=1, mapping="swapped", seed=41, width=2),
    Case("long_i16_a1s2", "long", DK.Int16, 2, 1, 1050000, pad=1, contrast=True, mapping="swapped", seed=42, route=R.CopyEngineStaged, kernel=2),
    Case("long_f32c_w16", "long", DK.Float32Complex, 2, 1, 2200000, mapping="swapped", seed=43, route=R.CopyEngineStaged, width=16),
    # ---- planted extremes: one A1S2 case per scalar type (planted() below)
    Case("planted_Int16", "planted", DK.Int16, 8, 2, 256, pad=37, contrast=True, seed=51, kernel=2),
    Case("planted_Float16", "planted", DK.Float16, 8, 2, 256, pad=5, contrast=True, seed=52, kernel=2),
    Case("planted_Float32", "planted", DK.Float32, 8, 2, 256, pad=3, contrast=True, seed=53, kernel=2),
]
CASES = {c.name: c for c in _CASES}
assert len(CASES) == len(_CASES)
SMALL = [c.name for c in _CASES if c.group == "small"]
LARGE = [c.name for c in _CASES if c.group == "large"]
LONG = [c.name for c in _CASES if c.group == "long"]
PLANTED = [c.name for c in _CASES if c.group == "planted"]

# (a, b, c) of out = a - b - c.  Int16: a - b - c leaves the int16 range and wraps mod 2^16.
PLANT_I16 = [(32767, -1, 0), (-32768, 1, 0), (32767, -32768, -32768), (-32768, 32767, 32767), (20000, -20000, 0), (-20000, 20000, 1),
             (32767, 0, -1), (0, 32767, 2), (-32768, 0, 1), (1, -32767, -32767), (32767, -32767, 32767), (-1, 32767, 1)]
# Float16: +-inf after the first subtraction (and no NaN: nothing infinite is subtracted from it); binary16 subnormal results, from
# subnormal and from normal operands; sums that round at a tie (spacing 2 above 2048: 2049 -> 2048, 2051 -> 2052, to even)
PLANT_F16 = [(65504, -65504, 0), (65504, -65504, 65504), (-65504, 65504, 0), (-65504, 65504, -1), (3 * 2.0 ** -24, 2.0 ** -24, 2.0 ** -24),
             (2.0 ** -14, 2.0 ** -15, 0), (2.0 ** -14, 2.0 ** -15, 2.0 ** -16), (-2.0 ** -14, -2.0 ** -15, 0), (2.0 ** -14, 2.0 ** -14 - 2.0 ** -24, 0),
             (2048, -1, 0), (2050, -1, 0), (2048, 0, -1), (-2050, 1, 0), (4096, -2, -2), (65504, -16, 0), (65504, -15.9921875, 0), (1, -2.0 ** -11, 0)]
PLANT_F16_EXPECT = [np.inf, np.inf, -np.inf, -np.inf, 2.0 ** -24, 2.0 ** -15, 2.0 ** -16, -2.0 ** -15, 2.0 ** -24,
                    2048, 2052, 2048, -2052, 4096, np.inf, 65504, 1]
# Float32: binary32 subnormal results; large cancellations; a tie at 2^24
PLANT_F32 = [(2.0 ** -126, 2.0 ** -127, 0), (1.5 * 2.0 ** -126, 2.0 ** -126, 0), (2.0 ** -126, 2.0 ** -126 - 2.0 ** -149, 0), (3 * 2.0 ** -149, 2.0 ** -149, 2.0 ** -149),
             (-2.0 ** -126, -2.0 ** -127, 0), (1e30, 1e30, 1), (1e30, 1, 1e30), (16777216, -1, 0), (16777218, -1, 0), (1, 2.0 ** -24, 2.0 ** -24),
             (3e38, -3e38, 0), (-3e38, 3e38, 1), (123456.789, 123456.78, 0)]
PLANT_F32_EXPECT = [2.0 ** -127, 2.0 ** -127, 2.0 ** -149, 2.0 ** -149, -2.0 ** -127, -1, 0, 16777216, 16777220, None,
                    np.inf, -np.inf, None]
PLANTS = {"planted_Int16": (PLANT_I16, [((a - b - c + 32768) % 65536) - 32768 for a, b, c in PLANT_I16]), "planted_Float16": (PLANT_F16, PLANT_F16_EXPECT), "planted_Float32": (PLANT_F32, PLANT_F32_EXPECT)}


def numpy_base(kind):
    return P.DATA_KIND_NUMPY[int(kind)]


def scalars(kind):
    return 2 if P.DATA_KIND_COMPLEX[int(kind)] else 1


@functools.lru_cache(maxsize=None)
def make(name, grid=GRID):
    """the case's Acquisition (cached: the tests share it and leave it unchanged).  grid: another voxel grid over the same region, the
    same RF (tests/test_gpu_ingest.py's compute-bound sequence: more voxels, so that the kernels lag behind the copies)"""
    c = CASES[name]
    z1 = 0.8 * cfg.SPEED_OF_SOUND * (c.samples / FS) / 2
    acq = cfg.rca(name, c.channels, c.transmits, c.samples, grid, (-2e-3, 0, 0.3 * z1), (2e-3, 0, z1), seed=1000 + c.seed, data_kind=c.kind,
                  stages=(S.Decode, S.DAS), decode=0, demodulate=False, fs=FS, fd=FD, pitch=PITCH, angles=np.linspace(-5, 5, c.transmits),
                  channel_shuffle=c.mapping == "shuffled", raw_pad=c.pad, contrast=c.contrast)
    if c.mapping == "swapped":          # the raw rows are noise: naming them the other way round is another valid acquisition
        for ch in range(c.channels):
            acq.bp.channel_mapping[ch] = c.channels - 1 - ch
    if c.group == "planted":
        triples, _ = PLANTS[name]
        k = c.samples * scalars(c.kind)
        rows = acq.rf.reshape(c.channels, -1)
        for i, (a, b, cc) in enumerate(triples):
            for row in range(c.channels):
                s = (i + 3 * row) % k                       # a few dozen samples of every row, not the same ones in every row
                rows[row, s], rows[row, k + s], rows[row, 2 * k + s] = a, b, cc
        assert not np.isnan(rows.astype(np.float64)).any()
    acq.rf.setflags(write=False)
    return acq


def planted_positions(name):
    """(mapped channel, sample, index into the triples) of every planted sample"""
    c = CASES[name]
    acq = make(name)
    k = c.samples * scalars(c.kind)
    out = []
    for ch in range(c.channels):
        row = int(acq.bp.channel_mapping[ch])
        for i in range(len(PLANTS[name][0])):
            out.append((ch, (i + 3 * row) % k, i))
    return out


def mapped_rf(acq, rf=None):
    """the RF slot after ingest, (channels, transmits x samples x scalars) of the data kind's scalar type"""
    bp = acq.bp
    base = numpy_base(bp.data_kind)
    n = scalars(bp.data_kind)
    Cn, A, Sn = int(bp.channel_count), int(bp.acquisition_count), int(bp.sample_count)
    raw = np.ascontiguousarray(acq.rf if rf is None else rf).view(base).reshape(int(bp.raw_data_dimensions[1]), int(bp.raw_data_dimensions[0]) * n)
    rows = raw[[int(bp.channel_mapping[ch]) for ch in range(Cn)]]
    row = A * Sn * n
    if not bp.contrast_mode:
        return np.ascontiguousarray(rows[:, :row])
    k = Sn * n
    out = np.zeros((Cn, row), base)
    with np.errstate(over="ignore", invalid="raise"):
        # numpy's typed array arithmetic: int16 wraps mod 2^16, float16 and float32 round once per operation
        first = rows[:, :k] - rows[:, k:2 * k]
        assert first.dtype == np.dtype(base)
        out[:, :k] = first - rows[:, 2 * k:3 * k]
    return out


def rf_checksum(mapped):
    data = np.ascontiguousarray(mapped).view(np.uint8).reshape(-1)
    words = data[: data.size // 8 * 8].view("<u8")
    with np.errstate(over="ignore"):
        return int((words * np.arange(1, words.size + 1, dtype=np.uint64)).sum(dtype=np.uint64))


def das_input_of(acq, mapped):
    """the DAS input the plan {Decode (None), DAS} hands on: the mapped RF as float32 / complex64, (channels, transmits, samples)"""
    bp = acq.bp
    shape = (int(bp.channel_count), int(bp.acquisition_count), int(bp.sample_count))
    f = mapped.astype(np.float32)                       # int16 and float16 convert exactly
    if scalars(bp.data_kind) == 2:
        return np.ascontiguousarray(f).view(np.complex64).reshape(shape)
    return f.reshape(shape)


@functools.lru_cache(maxsize=None)
def burst_case():
    """one frame of the large burst: 32 x 8 x 4096 Int16 + 2 samples of padding per row, 2 MiB -- under the copy-engine threshold alone,
    over it as five frames"""
    z1 = 0.8 * cfg.SPEED_OF_SOUND * (4096 / FS) / 2
    acq = cfg.rca("burst_2MiB", 32, 8, 4096, GRID, (-2e-3, 0, 0.3 * z1), (2e-3, 0, z1), seed=1061, data_kind=DK.Int16, stages=(S.Decode, S.DAS),
                  decode=0, demodulate=False, fs=FS, fd=FD, pitch=PITCH, angles=np.linspace(-5, 5, 8), channel_shuffle=True, raw_pad=2)
    acq.rf.setflags(write=False)
    return acq


def burst_frames(acq, n):
    """n different raw frames of one acquisition: frame k is the case's RF with every raw row rotated by 7 k + 1 scalars (noise: as
    valid a frame as the first), frame 0 the case's own"""
    return np.ascontiguousarray(np.stack([acq.rf if k == 0 else np.roll(acq.rf, 7 * k + 1, axis=1) for k in range(n)]))
