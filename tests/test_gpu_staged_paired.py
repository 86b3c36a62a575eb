"""The channel-paired form of the LDS-staged kernel (das_staged.hip, BfSeparableArgs.uniform = 2): 32 x 32 tiles with 32-sample
windows, two voxels per lane, transmit delays and phasors from a global table through scalar loads, the LDS holding two channels'
windows of one group of transmits at a time.  Against the oracle; range-checked loop bit-identical to the normal run; against the
transmit tables in LDS (STAGED_NOUNIFORM: the channels are summed in another order, so within 1e-4 of the peak, not bit-equal);
repeat frames and slabs bit-identical."""
import numpy as np
import pytest

from ogl_beamforming_amd import configs as cfg
from tests import cases, draws
from tests.das_push import compare, run, same_bits, use_devices
from tests.parity import reference

pytestmark = pytest.mark.gpu

LO3, HI3 = cases.LO3, cases.HI3

# beyond the named cases: transmit counts whose padded table needs two groups (76 = 40 + 36 as config 4; 68 = 36 + 32 with an odd
# count), an odd channel count (the last pair's zero partner) on a ragged grid, RF rows too short for the deep voxels (the checked
# loop).  (Focused transmits: their spread fits no 32 x 32 tile's 32-sample window on these grids -- the form is not planned.)
EXTRA = {
    "paired_two_groups": lambda: cfg.rca("paired_two_groups", 32, 75, 512, (150, 36, 2), LO3, HI3, seed=61, orientation=0x12, cw=True,
                                         f_number=0.6, angles=np.linspace(-12, 12, 75)),
    "paired_uneven_odd_channels": lambda: cfg.rca("paired_uneven_odd_channels", 33, 67, 512, (45, 150, 2), LO3, HI3, seed=62,
                                                  orientation=0x21, cw=True, f_number=0.6, angles=np.linspace(-12, 12, 67)),
    "paired_short_rows": lambda: cfg.rca("paired_short_rows", 32, 66, 384, (150, 40, 2), LO3, HI3, seed=64, orientation=0x12, cw=True,
                                         f_number=0.6, angles=np.linspace(-12, 12, 66)),
}
NAMED = ["config4_small", "rca_staged_fine"]


def make(name):
    return EXTRA[name]() if name in EXTRA else cases.make(name)


@pytest.mark.parametrize("name", NAMED + sorted(EXTRA))
def test_paired_staged_kernel(name, bflib, oracle, hooks):
    acq = make(name)
    lib = bflib.library()
    hooks.set("STAGED_SHAPE", "5,5,5")
    lib.beamformer_hip_set_das_path(3)
    try:
        _, _, _, _, d = bflib.describe_das(acq.bp, acq.filters)
        paired, path, _ = run(bflib, acq)
        assert path == 2 and d.uniform_tables == 2 and d.u_shift == 5 and d.v_shift == 5 and d.window_samples == 32
        again, _, _ = run(bflib, acq)
        assert same_bits(paired, again)                          # repeat frames
        hooks.set("STAGED_CHECKED")
        checked, path_checked, violations = run(bflib, acq)
        assert path_checked == 2 and violations == 0
        assert same_bits(paired, checked)                        # every term range-checked: the same arithmetic
        lib.beamformer_hip_set_hook(b"STAGED_CHECKED", None)
        hooks.set("STAGED_NOUNIFORM")
        assert bflib.describe_das(acq.bp, acq.filters)[4].uniform_tables == 0
        in_lds, path_lds, _ = run(bflib, acq)
        assert path_lds == 2
    finally:
        lib.beamformer_hip_set_das_path(0)
    ok = ~np.isnan(in_lds)
    assert np.array_equal(np.isnan(paired), ~ok)
    scale = np.max(np.abs(in_lds[ok]))
    assert np.max(np.abs(paired[ok] - in_lds[ok])) <= 1e-4 * scale
    ref, _, flags = reference(oracle, acq)
    compare(paired, ref, acq, flags, path=path)


PAIRED_DRAWS = []          # (seed, uniform_tables the plan chose, DAS path of the frame, planes re-routed by the row-end rule)


@pytest.mark.parametrize("seed", range(24))
def test_random_draws_on_the_paired_staged_kernel(seed, bflib, oracle, hooks):
    """tests/draws.py draw_paired: everything test_paired_staged_kernel asks of its fixed cases, on random draws -- one or two transmit
    groups, padded transmit counts, odd channel counts, ragged tiles, short rows (the deepest plane on the gather kernel) -- and the
    oracle's frame from draws the paired form does not take (more than two groups)"""
    acq = draws.draw_paired(seed)
    lib = bflib.library()
    hooks.set("STAGED_SHAPE", "5,5,5")
    lib.beamformer_hip_set_das_path(3)
    try:
        _, _, _, _, d = bflib.describe_das(acq.bp, acq.filters)
        form = int(d.uniform_tables)
        paired, path, violations = run(bflib, acq)
        PAIRED_DRAWS.append((seed, form, path, int(d.row_end_planes)))
        if form == 2:
            assert path == 2 and d.u_shift == 5 and d.v_shift == 5 and d.window_samples == 32
            again, _, _ = run(bflib, acq)
            assert same_bits(paired, again)                      # repeat frames
            hooks.set("STAGED_CHECKED")
            checked, path_checked, violations = run(bflib, acq)
            assert path_checked == 2 and violations == 0
            assert same_bits(paired, checked)                    # every term range-checked: the same arithmetic
            hooks.clear("STAGED_CHECKED")
            hooks.set("STAGED_NOUNIFORM")
            assert bflib.describe_das(acq.bp, acq.filters)[4].uniform_tables == 0
            in_lds, path_lds, _ = run(bflib, acq)
            assert path_lds == 2
    finally:
        lib.beamformer_hip_set_das_path(0)
    ref, _, flags = reference(oracle, acq)
    compare(paired, ref, acq, flags, path=path)
    if form == 2:
        ok = ~np.isnan(in_lds)
        assert np.array_equal(np.isnan(paired), ~ok)
        scale = np.max(np.abs(in_lds[ok]))
        assert np.max(np.abs(paired[ok] - in_lds[ok])) <= 1e-4 * scale


def test_random_draws_reach_the_paired_form():
    """the draws above are worth their name only if most of them ran the channel-paired form"""
    ran = [seed for seed, form, path, _ in PAIRED_DRAWS if form == 2 and path == 2]
    print(f"paired-form draws: {len(ran)} of {len(PAIRED_DRAWS)}; with planes re-routed by the row-end rule: "
          f"{sorted(seed for seed, form, _, planes in PAIRED_DRAWS if form == 2 and planes)}; other forms (seed, uniform_tables, path): "
          f"{[(seed, form, path) for seed, form, path, _ in PAIRED_DRAWS if form != 2]}")
    assert len(ran) >= 18, PAIRED_DRAWS


@pytest.mark.parametrize("name, count", [("paired_two_groups", 2), ("config4_small", 3)])
def test_paired_staged_kernel_slabs(name, count, bflib, hooks):
    """a slab of planes takes the same form and gives the same bits as those planes of the whole frame"""
    acq = make(name)
    lib = bflib.library()
    hooks.set("STAGED_SHAPE", "5,5,5")
    lib.beamformer_hip_set_das_path(3)
    try:
        use_devices(lib, [0])
        one, path, _ = run(bflib, acq)
        assert path == 2
        use_devices(lib, [0] * count)
        many = bflib.beamform(acq.bp, acq.rf, acq.filters).copy()
    finally:
        use_devices(lib, [0])
        lib.beamformer_hip_set_das_path(0)
    assert same_bits(one, many)
