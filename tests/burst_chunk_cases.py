"""The bursts that cross a chunk of the filters' launches (csrc/stages.hip launch_frame_chunks): 257 frames of 256 channels, where a
launch holds 65535 // 256 = 255 frames -- frames 0..254 go in the first launch, frames 255 and 256 in the second.  A plain module (no
pytest marker, no device): tests/test_gpu_stages_burst.py runs them on the device and tests/test_burst_host.py guards, on the CPU, that
they still cross the chunk."""
import numpy as np

from ogl_beamforming_amd import configs as cfg
from ogl_beamforming_amd import params as P

S = P.ShaderKind
FRAMES, CHANNELS, SOURCES = 257, 256, 4
CHUNK = 65535 // CHANNELS                         # the frames of one launch
FS, FD, PITCH = 25e6, 6.25e6, 0.3e-3
SAMPLES = 128
POINTS = (8, 1, 8)


def _depth(samples, rate):
    """0.8 of the depth whose echo arrives with the last of `samples` samples taken at `rate`"""
    return 0.8 * cfg.SPEED_OF_SOUND * (samples / rate) / 2


def demodulate_das():
    """Demodulate -> DAS: Int16, decimation 2, one unfocused transmit (the 256-thread filter form, one row per channel)"""
    z1 = _depth(SAMPLES // 4 // 2, FS / 4)        # 32 DAS samples at fs / 4, of which the filter computes the first 16
    acq = cfg.rca("chunk_demodulate_das", CHANNELS, 1, SAMPLES, POINTS, (-1e-3, 0, 0.4 * z1), (1e-3, 0, z1), seed=9100,
                  kind=P.AcquisitionKind.Flash, orientation=0x02, single=True, stages=(S.Demodulate, S.DAS), decimation=2,
                  fs=FS, fd=FD, pitch=PITCH)
    acq.filters = [cfg.kaiser_filter(FS / 2, FD / 2)]
    return acq


def demodulate_decode_das():
    """Demodulate -> Decode -> DAS with 4 transmits: the filter stores in Decode's layout through its transposing 1024-thread form"""
    z1 = _depth(SAMPLES // 2, FS / 2)
    return cfg.rca("chunk_demodulate_decode_das", CHANNELS, 4, SAMPLES, POINTS, (-1e-3, 0, 0.4 * z1), (1e-3, 0, z1), seed=9101,
                   stages=(S.Demodulate, S.Decode, S.DAS), decode=1, fs=FS, fd=FD, pitch=PITCH, angles=np.linspace(-5, 5, 4))


def decode_hilbert_das():
    """Decode -> Hilbert -> DAS: real Int16, one transmit, decode mode none (the planner drops the Decode)"""
    z1 = _depth(SAMPLES, FS)
    acq = cfg.rca("chunk_decode_hilbert_das", CHANNELS, 1, SAMPLES, POINTS, (-1e-3, 0, 0.4 * z1), (1e-3, 0, z1), seed=9102,
                  stages=(S.Decode, S.DAS), decode=0, fs=FS, fd=FD, pitch=PITCH)
    acq.bp.compute_stages[1], acq.bp.compute_stages[2] = int(S.Hilbert), int(S.DAS)
    acq.bp.compute_stages_count = 3
    return acq


CASES = {"demodulate_das": demodulate_das, "demodulate_decode_das": demodulate_decode_das, "decode_hilbert_das": decode_hilbert_das}
NEEDS_HILBERT = {"decode_hilbert_das"}


def assignment(seed):
    """which of the SOURCES distinct RF frames each of the FRAMES frames of the burst is: a seeded draw without a period, redrawn until
    the frames around the chunk boundary (254, 255, 256) come from three different sources and frames 255 and 256 -- the second launch's
    first two -- differ from frames 0 and 1: a chunk that started again at the beginning would otherwise show nothing"""
    rng = np.random.default_rng(seed)
    while True:
        a = rng.integers(0, SOURCES, FRAMES)
        if len({a[CHUNK - 1], a[CHUNK], a[CHUNK + 1]}) == 3 and a[CHUNK] != a[0] and a[CHUNK + 1] != a[1] and len(set(a)) == SOURCES:
            return a
