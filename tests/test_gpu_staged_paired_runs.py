"""RUNS of channel pairs in the channel-paired staged kernel (das_staged.hip): a wave chooses per channel pair what it does -- nothing
(the f-number culls both channels for all its lanes), the plain loop, or the range-checked loop (some lane can leave the RF row) -- and
stays inside one instantiation of its rounds for as long as the next pair's case is the same, at most to the end of the chunk.  A run
requests its first pair's windows itself and its last pair requests none, so every change of case is a place where staging, the
voxel's sums and the look-ahead of the next pair's case have to hand over correctly.

Which planes the kernel gets matters here: the host gives the staged kernels only planes whose IN-APERTURE terms provably stay clear
of the row ends (decide_das_parts, das_select.cpp) and sends the others to the kernel behind them.  So on a plane this kernel really
runs no kept lane is ever unsafe; a wave takes the range-checked loop there because of lanes the f-number CULLS: the receive table
decides "can leave the row" for every lane, kept or not, and one such lane makes its wave's pair range-checked.  The cases are small
frames of two planes, both kept by the paired kernel (row_end_planes == 0 is asserted, in the plan and in the frame's timings):

  * a shallow first plane: the f-number keeps only the channels near a tile and nothing comes near a row end, so over the channel
    pairs a wave goes skip -> plain -> skip;
  * a second plane whose in-aperture bound ends four samples short of the row end, on tiles 2.6 mm wide along the receive axis: the
    channel pairs at the edge of a tile's aperture have kept lanes next to culled lanes up to 2.6 mm further out, whose receive path
    is a dozen samples longer and leaves the row: skip -> checked -> plain -> checked -> skip.
    (With this geometry -- the outermost kept channels are the ones that come near the row's END, as the issue builds it -- the
    range-checked case sits at the outer ends of the kept channels, not in their middle: "plain -> checked -> plain" would need the
    NEAREST channels to be the unsafe ones, delays short of the row's start.  Together the two planes have all six changes between
    the three cases, which is what the hand-over code can get wrong.)

`modes_of` restates the kernel's decision in float64 (the f-number test and the row-end test of the receive table with the tile-wide
extremes of the transmit delay) from the parameters and from what the library's plan says the DAS stage sees (sample count, sampling
frequency and time offset behind the demodulation); test_cases_change_case_inside_a_chunk asserts with it, with no GPU, that every
case has all six changes between consecutive pairs of one chunk, and test_cases_are_planned_in_the_paired_form that the plan is the
paired form for BOTH planes -- so the GPU test cannot pass by running another kernel or frames without runs.  On the GPU each case is
judged as the other paired tests judge theirs: tests/parity.compare against the oracle, no window violation, and once more with every
term range-checked (STAGED_CHECKED: one run per chunk), bit-equal."""
import ctypes as C

import numpy as np
import pytest

from ogl_beamforming_amd import configs as cfg
from ogl_beamforming_amd import lib as bf
from ogl_beamforming_amd import params as P
from tests.das_push import compare, last_timings, lds_bytes, plan, run, same_bits
from tests.parity import reference

PITCH, FS, F_NUMBER = 0.3e-3, 25e6, 0.8
U_SPAN, V_SPAN = 4e-3, 1.2e-3              # half extents of the grid along the receive and the transmit axis
U_POINTS, V_POINTS = 96, 36                # 3 x 2 tiles of 32 x 32; a tile is 2.6 mm wide along the receive axis


def rca(name, channels, transmits, samples, z_planes, seed, orientation, cw):
    """orientation 0x12: the receive axis is x; 0x21: y"""
    along_x = orientation == 0x12
    span = (U_SPAN, V_SPAN) if along_x else (V_SPAN, U_SPAN)
    points = (U_POINTS, V_POINTS, 2) if along_x else (V_POINTS, U_POINTS, 2)
    lo, hi = (-span[0], -span[1], z_planes[0]), (span[0], span[1], z_planes[1])
    return cfg.rca(name, channels, transmits, samples, points, lo, hi, seed=seed, orientation=orientation, cw=cw, f_number=F_NUMBER,
                   pitch=PITCH, fs=FS, angles=np.linspace(-12, 12, transmits))


# name: (acquisition, (g0, g1) the split of the padded transmit count, the axis of `points` along the receive axis, the two planes,
#        channel pairs, channels per chunk)
CASES = {
    # one group, an odd number of real transmits, 64 channels in one chunk
    "runs_one_group": (lambda: rca("runs_one_group", 64, 11, 384, (4e-3, 9.5e-3), 91, 0x12, True), (12, 0), 0, (4e-3, 9.5e-3), 32, 64),
    # config 4's split of 75 transmits (48 + 28, the second group ends in an odd transmit), the other orientation, chunks of 16
    "runs_two_groups": (lambda: rca("runs_two_groups", 62, 75, 384, (4e-3, 9.5e-3), 92, 0x21, True), (48, 28), 1, (4e-3, 9.5e-3), 31, 16),
    # no coherency weighting, an odd channel count (the last pair's zero partner ends the last run)
    "runs_odd_channels": (lambda: rca("runs_odd_channels", 63, 8, 384, (4.5e-3, 9.4e-3), 93, 0x12, False), (8, 0), 0, (4.5e-3, 9.4e-3), 32, 63),
}
SKIP, PLAIN, CHECKED = 0, 1, 2
ALL_CHANGES = {(a, b) for a in (SKIP, PLAIN, CHECKED) for b in (SKIP, PLAIN, CHECKED) if a != b}


def das_stage_of(acq):
    """(plan of the DAS launch, samples per row, sampling frequency and time offset the DAS stage sees) -- needs no device"""
    d = plan(acq)                                                # (pushes the parameters: the stage plan below is theirs)
    stages = P.HipPlan()
    assert bf.library().beamformer_hip_describe_plan(0, C.byref(stages))
    return d, int(stages.das_samples), float(stages.das_sampling_frequency), float(stages.das_time_offset)


def modes_of(acq, u_points_axis, z_planes, chunk, samples, fs, t0):
    """{(tile along u, tile along v, plane): [case of each channel pair]} and the changes of case between consecutive pairs of one
    chunk: the receive table's f-number test and row-end test (das_staged.hip) in float64"""
    bp = acq.bp
    channels, transmits = int(bp.channel_count), int(bp.acquisition_count)
    c = cfg.SPEED_OF_SOUND
    half = (channels - 1) / 2 * PITCH
    assert [int(bp.output_points[i]) for i in (u_points_axis, 1 - u_points_axis)] == [U_POINTS, V_POINTS]
    u = np.linspace(-U_SPAN, U_SPAN, U_POINTS) + half            # transducer coordinate along the receive axis
    v_world = np.linspace(-V_SPAN, V_SPAN, V_POINTS)             # world coordinate along the transmit axis
    angles = np.deg2rad([float(bp.steering_angles[a]) for a in range(transmits)])
    out, changes = {}, set()
    for plane, z in enumerate(z_planes):
        for tv in range((V_POINTS + 31) // 32):
            rows = v_world[tv * 32:(tv + 1) * 32]                  # the tile's extremes of the absolute transmit delay
            t = ((rows[None, :] * np.sin(angles)[:, None] + z * np.cos(angles)[:, None]) / c + t0) * fs
            for tu in range((U_POINTS + 31) // 32):
                lanes = u[tu * 32:(tu + 1) * 32]
                dx = lanes[None, :] - (np.arange(channels) * PITCH)[:, None]
                kept = np.abs(dx) * F_NUMBER / z < 0.5
                r = np.sqrt(dx * dx + z * z) / c * fs
                unsafe = (r + t.min() < 0) | (r + t.max() >= samples - 1)     # every lane, kept or culled
                row = []
                for k in range((channels + 1) // 2):
                    pair = slice(2 * k, min(2 * k + 2, channels))
                    row.append(SKIP if not kept[pair].any() else CHECKED if unsafe[pair].any() else PLAIN)
                out[(tu, tv, plane)] = row
                changes |= {(a, b) for k, (a, b) in enumerate(zip(row, row[1:])) if a != b and (2 * k) // chunk == (2 * k + 2) // chunk}
    return out, changes


@pytest.mark.parametrize("name", sorted(CASES))
def test_cases_are_planned_in_the_paired_form(name):
    """the paired form, in the split, pair count and chunk the case names -- and for both planes: none goes to the kernel behind it"""
    make, (g0, g1), _, _, pairs, chunk = CASES[name]
    acq = make()
    d = plan(acq)
    assert d.uniform_tables == 2 and d.u_shift == 5 and d.v_shift == 5 and d.window_samples == 32
    assert int(d.row_end_planes) == 0 and int(d.row_ends) == 0
    a4 = (int(acq.bp.acquisition_count) + 3) // 4 * 4
    assert g0 + g1 == a4 and int(d.lds_bytes) == lds_bytes(g0, int(d.channel_chunk), a4)
    assert (int(acq.bp.channel_count) + 1) // 2 == pairs and int(d.channel_chunk) == chunk


@pytest.mark.parametrize("name", sorted(CASES))
def test_cases_change_case_inside_a_chunk(name):
    """every case has, between consecutive channel pairs of one chunk, all six changes between skip, plain and range-checked -- and
    on the shallow plane the whole sequence skip -> plain -> skip, on the deep one skip -> checked -> plain -> checked -> skip, with
    at least two range-checked pairs at either end (the model is float64: one pair of slack)"""
    make, _, u_points_axis, z_planes, _, _ = CASES[name]
    acq = make()
    d, samples, fs, t0 = das_stage_of(acq)
    assert int(d.row_end_planes) == 0
    modes, changes = modes_of(acq, u_points_axis, z_planes, int(d.channel_chunk), samples, fs, t0)
    assert changes == ALL_CHANGES, (sorted(ALL_CHANGES - changes), int(d.channel_chunk))

    def runs(row):
        return tuple(m for i, m in enumerate(row) if i == 0 or m != row[i - 1])
    shallow = {runs(row) for (tu, tv, plane), row in modes.items() if plane == 0}
    assert shallow == {(SKIP, PLAIN, SKIP)}, shallow
    centre = [row for (tu, tv, plane), row in modes.items() if plane == 1 and tu == 1]
    for row in centre:
        assert runs(row) == (SKIP, CHECKED, PLAIN, CHECKED, SKIP), row
        first_plain, last_plain = row.index(PLAIN), len(row) - 1 - row[::-1].index(PLAIN)
        assert row[:first_plain].count(CHECKED) >= 2 and row[last_plain + 1:].count(CHECKED) >= 2, row


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_paired_staged_kernel_over_changes_of_case(name, bflib, oracle, hooks):
    make, (g0, g1), _, _, pairs, chunk = CASES[name]
    acq = make()
    lib = bflib.library()
    hooks.set("STAGED_SHAPE", "5,5,5")
    lib.beamformer_hip_set_das_path(3)
    try:
        d = bflib.describe_das(acq.bp, acq.filters)[4]
        paired, path, violations = run(bflib, acq)
        assert path == 2 and d.uniform_tables == 2 and d.u_shift == 5 and d.v_shift == 5 and d.window_samples == 32
        assert (int(acq.bp.channel_count) + 1) // 2 == pairs and int(d.channel_chunk) == chunk and violations == 0
        # both planes on the paired kernel: none re-routed by the row-end rule
        assert int(d.row_end_planes) == 0 and int(last_timings(bflib).das_row_end_planes) == 0
        again, _, _ = run(bflib, acq)
        assert same_bits(paired, again)                          # repeat frames
        hooks.set("STAGED_CHECKED")
        checked, path_checked, violations = run(bflib, acq)
        assert path_checked == 2 and violations == 0 and int(last_timings(bflib).das_row_end_planes) == 0
        hooks.clear("STAGED_CHECKED")
    finally:
        lib.beamformer_hip_set_das_path(0)
    ref, _, flags = reference(oracle, acq)
    compare(paired, ref, acq, flags, path=path)
    compare(checked, ref, acq, flags, path=path_checked)         # once more under STAGED_CHECKED: one run per chunk
    assert same_bits(paired, checked)                            # and the same arithmetic
