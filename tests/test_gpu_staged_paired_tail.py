"""Where the transmits of the channel-paired staged kernel (das_staged.hip) END: the transmit table and the LDS blocks are laid out for
the count padded to a multiple of 4, a group's batches take two transmits each, and the plain loop requests the table row of the next
batch behind the current batch's last rotate-accumulate while the group's last batch, behind the loop, requests none.  So the cases
are chosen by what the last batches of a group hold: real transmits only, one real and one padding transmit (an odd real count), or
padding alone.

Cases (A4 = A rounded up to 4; two groups split the padded count, the first is a multiple of 4 and holds real transmits only, so an
odd real count can only sit in a single group or in the second of two -- never in both groups of one frame):

  A = 7   -> 8          one group, odd count (3 pairs + 1), A % 4 = 3, odd channel count, ragged grid
  A = 8                 one group, no padding, the last batch a whole pair, A % 4 = 0, no coherency weighting
  A = 9   -> 12         one group, odd count with a whole padding batch behind it, A % 4 = 1
  A = 33  -> 36         one group of three staging passes, odd count, A % 4 = 1, odd channel count, no coherency weighting
  A = 61  -> 64 = 32+32 group 1 holds 29 real transmits (odd) and a padding batch, A % 4 = 1
  A = 64     = 32+32    two groups, no padding, A % 4 = 0
  A = 66  -> 68 = 48+20 group 1 holds 18 real transmits (even) and one padding batch, A % 4 = 2; RF rows too short for the deep
                        voxels: waves run the range-checked loop in the normal frame
  A = 75  -> 76 = 48+28 config 4's split: group 1 holds 27 real transmits (odd), A % 4 = 3, odd channel count

Each asks what tests/test_gpu_staged_paired.py asks of its cases: the oracle through compare() at its tolerance, bit-equal on repeat,
bit-equal with every term range-checked and no window violation, within 1e-4 of the peak of the form with the tables in LDS."""
import numpy as np
import pytest

from ogl_beamforming_amd import configs as cfg
from tests import cases
from tests.das_push import compare, lds_bytes, plan, run, same_bits
from tests.parity import reference

LO3, HI3 = cases.LO3, cases.HI3


def rca(name, channels, transmits, samples, points, seed, orientation, cw):
    return cfg.rca(name, channels, transmits, samples, points, LO3, HI3, seed=seed, orientation=orientation, cw=cw, f_number=0.6,
                   angles=np.linspace(-12, 12, transmits))


# name: (acquisition, (g0, g1) the split of the padded count, real transmits of the last group)
CASES = {
    "a7_one_group_odd": (lambda: rca("tail_a7", 33, 7, 512, (45, 150, 2), 81, 0x21, True), (8, 0), 7),
    "a8_one_group_whole": (lambda: rca("tail_a8", 32, 8, 512, (150, 36, 2), 82, 0x12, False), (8, 0), 8),
    "a9_one_group_odd_padding_batch": (lambda: rca("tail_a9", 32, 9, 512, (150, 36, 2), 83, 0x12, True), (12, 0), 9),
    "a33_one_group_three_passes_odd": (lambda: rca("tail_a33", 31, 33, 512, (150, 40, 2), 84, 0x12, False), (36, 0), 33),
    "a61_second_group_odd": (lambda: rca("tail_a61", 32, 61, 512, (150, 36, 2), 85, 0x12, True), (32, 32), 29),
    "a64_two_groups_whole": (lambda: rca("tail_a64", 32, 64, 512, (40, 150, 2), 86, 0x21, True), (32, 32), 32),
    "a66_second_group_even_short_rows": (lambda: rca("tail_a66", 32, 66, 384, (150, 40, 2), 87, 0x12, True), (48, 20), 18),
    "a75_second_group_odd": (lambda: rca("tail_a75", 33, 75, 512, (45, 150, 2), 88, 0x21, True), (48, 28), 27),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_tail_cases_are_planned_in_the_paired_form(name):
    """every case runs the channel-paired form, in the split its name says, and ends where its name says"""
    make, (g0, g1), last_real = CASES[name]
    acq = make()
    d = plan(acq)
    assert d.uniform_tables == 2 and d.u_shift == 5 and d.v_shift == 5 and d.window_samples == 32
    count = int(acq.bp.acquisition_count)
    a4 = (count + 3) // 4 * 4
    assert g0 + g1 == a4 and int(d.lds_bytes) == lds_bytes(g0, int(d.channel_chunk), a4)
    assert last_real == (count - g0 if g1 else count) and 0 < last_real <= (g1 or g0)


def test_tail_cases_cover_the_ends_of_a_group():
    counts = [int(make().bp.acquisition_count) for make, _, _ in CASES.values()]
    assert {c % 4 for c in counts} == {0, 1, 2, 3}
    one_group_odd = [n for n, (_, (g0, g1), last) in CASES.items() if not g1 and last % 2]
    second_group_odd = [n for n, (_, (g0, g1), last) in CASES.items() if g1 and last % 2]
    second_group_even_padded = [n for n, (_, (g0, g1), last) in CASES.items() if g1 and last % 2 == 0 and last < g1]
    assert one_group_odd and second_group_odd and second_group_even_padded
    channels = {int(make().bp.channel_count) % 2 for make, _, _ in CASES.values()}
    weighting = {bool(make().bp.coherency_weighting) for make, _, _ in CASES.values()}
    assert channels == {0, 1} and weighting == {False, True}


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_paired_staged_kernel_at_the_end_of_a_group(name, bflib, oracle, hooks):
    acq = CASES[name][0]()
    lib = bflib.library()
    hooks.set("STAGED_SHAPE", "5,5,5")
    lib.beamformer_hip_set_das_path(3)
    try:
        d = bflib.describe_das(acq.bp, acq.filters)[4]
        paired, path, _ = run(bflib, acq)
        assert path == 2 and d.uniform_tables == 2 and d.u_shift == 5 and d.v_shift == 5 and d.window_samples == 32
        again, _, _ = run(bflib, acq)
        assert same_bits(paired, again)                          # repeat frames
        hooks.set("STAGED_CHECKED")
        checked, path_checked, violations = run(bflib, acq)
        assert path_checked == 2 and violations == 0
        assert same_bits(paired, checked)                        # every term range-checked: the same arithmetic
        hooks.clear("STAGED_CHECKED")
        hooks.set("STAGED_NOUNIFORM")
        assert bflib.describe_das(acq.bp, acq.filters)[4].uniform_tables == 0
        in_lds, path_lds, _ = run(bflib, acq)
        assert path_lds == 2
    finally:
        lib.beamformer_hip_set_das_path(0)
    ok = ~np.isnan(in_lds)
    assert np.array_equal(np.isnan(paired), ~ok)
    scale = np.max(np.abs(in_lds[ok]))
    worst = np.max(np.abs(paired[ok] - in_lds[ok]))
    print(f"{name}: worst difference to the LDS-table form {worst / scale:.3e} of the peak")
    assert worst <= 1e-4 * scale
    ref, _, flags = reference(oracle, acq)
    compare(paired, ref, acq, flags, path=path)
