"""The channel-paired staged kernel (das_staged.hip) over the group splits bf_staged_paired_split (bf_kernels.h) produces: the transmits
are staged in one group or in two, the first sized to whole staging passes (16 transmits each), and a wave converts and stores in a pass
only if its transmit belongs to the group.  One case per kind of split, each against the oracle with the per-voxel bars of
tests/parity.py, repeated bit for bit, and under the range-checked loop (STAGED_CHECKED) with no window violation and the same bits.

  one group, last pass partial        44 transmits = 44            (3 passes, the third holds 12 transmits' blocks)
  two groups of whole passes          80 = 48 + 32                 (3 + 2 passes)
  last group ending in a short pass   68 = 48 + 20                 (3 + 2 passes, the last holds 4 transmits' blocks)
  count not a multiple of 4           75 -> 76 = 48 + 28           (config 4's split; one padding transmit with a zero window)
  odd channel count                   33 channels, 85 -> 88 = 48 + 40   (the last pair's zero partner in both groups)

(A last group of fewer than 16 transmits -- shorter than one pass -- is a split the rule never chooses: a one-pass group runs as two
passes, and whenever two groups are needed a more even split costs no more passes; tests/test_staged_paired_split.py checks the rule
for every transmit count.  Its nearest kin, a group whose LAST pass is short, are the 68- and 44-transmit cases.)"""
import numpy as np
import pytest

from ogl_beamforming_amd import configs as cfg
from tests import cases
from tests.das_push import compare, last_das_path, last_timings, same_bits
from tests.parity import reference

pytestmark = pytest.mark.gpu

LO3, HI3 = cases.LO3, cases.HI3


def rca(name, channels, transmits, points, seed, orientation):
    return cfg.rca(name, channels, transmits, 512, points, LO3, HI3, seed=seed, orientation=orientation, cw=True, f_number=0.6,
                   angles=np.linspace(-12, 12, transmits))


# name: (acquisition, (g0, g1) the split must give for the plan's chunk of channels)
CASES = {
    "one_group_partial_pass": (lambda: rca("groups_one", 32, 44, (150, 36, 2), 71, 0x12), (44, 0)),
    "two_groups_whole_passes": (lambda: rca("groups_whole", 32, 80, (150, 36, 2), 72, 0x12), (48, 32)),
    "last_group_short_last_pass": (lambda: rca("groups_short", 32, 68, (40, 150, 2), 73, 0x21), (48, 20)),
    "transmits_not_a_multiple_of_4": (lambda: rca("groups_padded", 32, 75, (45, 150, 2), 74, 0x21), (48, 28)),
    "odd_channel_count": (lambda: rca("groups_odd", 33, 85, (150, 40, 2), 75, 0x12), (48, 40)),
}


def lds_bytes(group, chunk, a4):
    """bf_staged_paired_lds_bytes (bf_kernels.h), restated"""
    return (16 * (group * 64 + 3) + 16 * (((chunk + 1) & ~1) << 5) + 4 * (a4 + 2 * (chunk + 2)) + 128 + 15) & ~15


def run(bflib, acq):
    frame = bflib.beamform(acq.bp, acq.rf, acq.filters).copy()
    return frame, last_das_path(bflib), last_timings(bflib).staged_window_violations


@pytest.mark.parametrize("name", sorted(CASES))
def test_paired_staged_kernel_group_splits(name, bflib, oracle, hooks):
    make, (g0, g1) = CASES[name]
    acq = make()
    lib = bflib.library()
    hooks.set("STAGED_SHAPE", "5,5,5")
    lib.beamformer_hip_set_das_path(3)
    try:
        d = bflib.describe_das(acq.bp, acq.filters)[4]
        assert d.uniform_tables == 2 and d.u_shift == 5 and d.v_shift == 5 and d.window_samples == 32
        a4 = (int(acq.bp.acquisition_count) + 3) // 4 * 4
        assert g0 + g1 == a4
        # the plan sized the LDS for the split this case is about (the larger group's windows) and leaves two blocks per CU
        assert int(d.lds_bytes) == lds_bytes(g0, int(d.channel_chunk), a4) <= 80 * 1024
        paired, path, _ = run(bflib, acq)
        assert path == 2
        again, _, _ = run(bflib, acq)
        assert same_bits(paired, again)                          # repeat frames
        hooks.set("STAGED_CHECKED")
        checked, path_checked, violations = run(bflib, acq)
        assert path_checked == 2 and violations == 0
        assert same_bits(paired, checked)                        # every term range-checked: the same arithmetic
    finally:
        lib.beamformer_hip_set_das_path(0)
    ref, _, flags = reference(oracle, acq)
    compare(paired, ref, acq, flags, path=path)
