"""The cases of tests/cases.py each DAS kernel takes.  FACTORED, HERCULES and TILE ask the library (beamformer_hip_describe_das) while this
module is imported: import it only where a list is needed."""
from ogl_beamforming_amd import params as P
from tests import cases


# geometries whose receive and transmit axes differ: the separable-delay fast path must pick
# them up on its own (das_separable.hip)
SEPARABLE = {"config4_small", "rca_vls_cw", "rca_sep_ragged_cubic", "rca_sep_real_nearest",
             "rca_staged_w64", "rca_staged_too_wide", "rca_staged_ragged", "rca_staged_auto", "rca_vls_staged", "rca_vls_staged_short_rows", "rca_staged_real", "rca_staged_real_short_rows", "rca_staged_real_narrow_cw", "rca_staged_cubic", "rca_staged_cubic_short_rows",
             "rca_staged_fine", "rca_staged_fine_vls_short_rows"}
# ... and of those, the ones with linear interpolation (complex or real samples) or cubic interpolation of complex samples whose
# delay spread fits an LDS window
# can run the LDS-staged kernel (das_staged.hip): automatically from STAGED_MIN_TRANSMITS transmits per
# channel (executor.cpp kStagedMinTransmits), on request (path 3) below that
STAGED = {"config4_small", "rca_staged_w64", "rca_staged_ragged", "rca_staged_auto", "rca_vls_staged", "rca_vls_staged_short_rows", "rca_staged_real", "rca_staged_real_short_rows", "rca_staged_real_narrow_cw", "rca_staged_cubic", "rca_staged_cubic_short_rows",
          "rca_sep_ragged_cubic", "rca_staged_fine", "rca_staged_fine_vls_short_rows"}
STAGED_MIN_TRANSMITS = 6


def factored_applies(acq):
    """whether das_factored.hip takes the frame when asked for (das path 4): the library says (beamformer_hip_describe_das)"""
    from ogl_beamforming_amd import lib
    L = lib.library()
    L.beamformer_hip_set_das_path(0x14)
    try:
        return lib.describe_das(acq.bp, acq.filters)[0] == 3
    finally:
        L.beamformer_hip_set_das_path(0)


def hercules_family(bp):
    return P.AcquisitionKind(bp.acquisition_kind) in (P.AcquisitionKind.HERCULES, P.AcquisitionKind.UHERCULES,
                                                      P.AcquisitionKind.HERO_PA)


HERCULES = sorted(n for n in cases.CASES if hercules_family(cases.make(n).bp))
FACTORED = sorted(n for n in cases.CASES if factored_applies(cases.make(n)))


def tile_candidates():
    from ogl_beamforming_amd import lib as bflib_mod
    out = []
    lib = bflib_mod.library()
    lib.beamformer_hip_set_das_path(0x14 | 0x100)
    try:
        for n in sorted(cases.CASES):
            acq = cases.make(n)
            if bflib_mod.describe_das(acq.bp, acq.filters)[0] == 5:
                out.append(n)
    finally:
        lib.beamformer_hip_set_das_path(0)
    return sorted(out)


TILE = tile_candidates()
