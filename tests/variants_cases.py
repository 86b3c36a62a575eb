"""The small blocks and candidate lists the variants tests share (tests/test_variants_host.py on the CPU, tests/test_gpu_variants.py
on the device): 16 channels x 2 transmits x 256 samples, an RCA_TPW (or Flash) block on a 24 x 1 x 40 grid -- 960 voxels: several
256-voxel tiles, a ragged last one, no multiple of the tile -- whose 256-sample rows reach just past the image at 1540 m/s, so that
a candidate's speed decides whether its terms come near the ends of the rows.  A plain module: no test, no device."""
import numpy as np

from ogl_beamforming_amd import configs as cfg
from ogl_beamforming_amd import lib
from ogl_beamforming_amd import params as P

I = P.InterpolationMode
D = P.DataKind
LO, HI = (-2.5e-3, 0.0, 3.0e-3), (2.5e-3, 0.0, 5.5e-3)
POINTS = (24, 1, 40)
PREFER, NO_KERNEL = P.HIP_DAS_PATH_PREFER_VARIANTS_KERNEL, P.HIP_DAS_PATH_NO_VARIANTS_KERNEL
INTERP = {"nearest": I.Nearest, "linear": I.Linear, "cubic": I.Cubic}


def block(interp="linear", iq=True, cw=False, flash=False, demodulate=False, seed=7100):
    """Float32 / Float32Complex RF straight into DAS (judged at 1e-4), or -- demodulate -- Int16 RF through Demodulate (2e-3)"""
    name = f"variants_{interp}_{'iq' if iq else 'real'}{'_cw' if cw else ''}{'_flash' if flash else ''}{'_demod' if demodulate else ''}"
    kind = dict(kind=P.AcquisitionKind.Flash, single=True) if flash else dict(kind=P.AcquisitionKind.RCA_TPW)
    if demodulate:
        return cfg.rca(name, 16, 2, 256, POINTS, LO, HI, seed=seed, interp=INTERP[interp], cw=cw, angles=np.array([-6.0, 6.0]), **kind)
    return cfg.rca(name, 16, 1 if flash else 2, 256, POINTS, LO, HI, seed=seed, interp=INTERP[interp], cw=cw, demodulate=False,
                   data_kind=D.Float32Complex if iq else D.Float32, angles=np.array([0.0]) if flash else np.array([-6.0, 6.0]), **kind)


LO3, HI3 = (-2.5e-3, -2.5e-3, 3.0e-3), (2.5e-3, 2.5e-3, 5.5e-3)


def forces_block():
    """16 channels x 8 transmits of FORCES on 16 x 16 x 32: single frames run the per-voxel factored kernel"""
    return cfg.forces("variants_forces", 16, 8, 256, (16, 16, 32), LO3, HI3, seed=7200, decode=0, data_kind=D.Float32,
                      stages=(P.ShaderKind.Decode, P.ShaderKind.DAS))


def separable_volume():
    """16 x 8 transmits steered along the rows, received along the columns, on 16 x 16 x 32: the separable-delay gather kernel"""
    return cfg.rca("variants_separable", 16, 8, 256, (16, 16, 32), LO3, HI3, seed=7201, orientation=0x12, demodulate=False,
                   data_kind=D.Float32Complex, angles=np.linspace(-8, 8, 8))


def candidates(bp):
    """K = 3: the speeds 1450 / 1540 / 1620 m/s, the second with a time offset shifted by 0.3 us, the third with half the f-number"""
    return [lib.variant_of(bp, speed_of_sound=1450.0),
            lib.variant_of(bp, speed_of_sound=1540.0, time_offset=bp.time_offset + 0.3e-6),
            lib.variant_of(bp, speed_of_sound=1620.0, f_number=bp.f_number / 2)]


def row_ends_of(bp, v, filters=()):
    """BeamformerHipDasDescription::row_ends of the block carrying the variant's values (no device needed)"""
    return int(lib.describe_das(lib.with_variant(bp, v), filters)[4].row_ends)


def slow_candidate(bp, filters=()):
    """the fastest of a ladder of low speeds at which some term of the block reaches an end of its 256-sample rows"""
    for speed in (1400.0, 1350.0, 1300.0, 1250.0, 1200.0, 1150.0, 1100.0, 1000.0, 900.0):
        v = lib.variant_of(bp, speed_of_sound=speed)
        if row_ends_of(bp, v, filters):
            return v
    raise AssertionError("no speed of the ladder brings a term to the end of a row")
