"""Child process of tests/test_gpu_frame_ops_contract.py: one `produce` operation of tests/frame_ops_table.py in a frame ring of
BEAMFORMER_HIP_FRAME_RING_BYTES = 1 MiB (the ring is sized once per process): 32 complex 64 x 1 x 64 frames of 32 KiB.  A burst of 16
and a mix 16 -> 15 leave 32 KiB at the end of the ring, and a call of the operation that makes 2 frames wraps to offset 0, clear of its
sources; another burst of 16 and a mix 16 -> 14 then fill the ring to its last byte, and every call on the 32 newest frames -- the two
frames at offset 0 among them -- would land on its own sources, or does not fit the ring at all: FrameSizeOverflow, and nothing has
changed; a call on the 14 newest then wraps to offset 0.  How the operation is called, how many frames a call makes and how they are
judged against its reference come from its record (FrameOp.ring_runs).
Started as python -m tests.frame_run_wrap_worker <operation> from the repository root (tests/scaffold.py run_ring_worker)."""
import ctypes as C
import os
import sys

import numpy as np

from ogl_beamforming_amd import configs as cfg, lib, params as P
from tests import variants_cases as vc
from tests.frame_info import newest_info as newest
from tests.frame_ops_table import PRODUCE


def main(name):
    op = {op.name: op for op in PRODUCE}[name]
    ring = int(os.environ["BEAMFORMER_HIP_FRAME_RING_BYTES"])
    assert ring == 1 << 20
    L = lib.library()
    L.beamformer_set_global_timeout(0xFFFFFFFF)
    acq = cfg.rca("frame_run_wrap", 16, 2, 256, (64, 1, 64), vc.LO, vc.HI, seed=8950, interp=P.InterpolationMode.Linear, demodulate=False,
                  data_kind=P.DataKind.Float32Complex, angles=np.array([-6.0, 6.0]), kind=P.AcquisitionKind.RCA_TPW)
    rng = np.random.default_rng(8951)
    rf = rng.normal(0.0, 1.0, (16,) + acq.rf.shape).astype(acq.rf.dtype)
    W = (rng.standard_normal((16, 16)) + 1j * rng.standard_normal((16, 16))).astype(np.complex64)
    two, refusals, last = op.ring_runs(rng, W)
    assert two.outputs == 2 and last.K == 14
    burst = lib.beamform_burst(acq.bp, rf, acq.filters).copy()                 # ids 0 .. 15 at offset 0 .. 512 KiB
    each = int(newest(L).size_bytes)
    base = int(newest(L).device_pointer) - 15 * each
    assert each == 64 * 64 * 8 and int(newest(L).frame_id) == 15 and 32 * each == ring

    # 16 -> 15: ids 16 .. 30 up to 992 KiB; two frames (64 KiB) do not fit behind them: the operation's run wraps to offset 0
    first, _ = lib.mix_last_frames(16, W[:15])
    mixed = lib.get_last_frames(acq.bp, 15).copy()
    assert first == 16 and int(newest(L).device_pointer) == base + 30 * each and lib.last_burst_info().first_frame_id == 0
    first, _ = two.call()
    out = lib.get_last_frames(acq.bp, 2).copy()
    assert first == 31 and int(lib.frame_info(31).device_pointer) == base and int(newest(L).device_pointer) == base + each
    wrapped = two.judge(out, mixed[15 - two.K:])
    print(f"wrapped: two frames of {op.name} at offset 0, worst error {wrapped:.4f} of its bound")
    assert np.array_equal(lib.copy_frame(31 - two.K).view(np.uint32), mixed[15 - two.K].view(np.uint32))     # a source of the run
    assert np.array_equal(lib.copy_frame(2).view(np.uint32), burst[2].view(np.uint32))          # the burst behind the run is still there
    for gone in (0, 1):
        raw = np.zeros(each // 4, np.float32)
        assert not L.beamformer_hip_copy_frame(gone, raw.ctypes.data_as(C.c_void_p), raw.nbytes) and lib.last_error()[0] == P.LibError.InvalidAccess
        assert not L.beamformer_hip_get_frame_info(gone, C.byref(P.HipFrameInfo()))

    # a burst (ids 33 .. 48, 64 .. 576 KiB) and a mix 16 -> 14 (ids 49 .. 62) fill the ring to its last byte
    lib.beamform_burst(acq.bp, rf, acq.filters)
    first, _ = lib.mix_last_frames(16, W[:14])
    assert first == 49 and int(newest(L).device_pointer) == base + 31 * each and int(newest(L).frame_id) == 62
    # the 32 newest frames, ids 31 .. 62, are the whole ring: whatever the call makes of them would lie on one of them
    newest_frames = lib.get_last_frames(acq.bp, 32).copy()
    before = bytes(newest(L))
    assert len(refusals) >= 2
    for change in refusals:
        call, untouched = op.bare(32, **change)
        assert not call(L)
        assert lib.last_error()[0] == P.LibError.FrameSizeOverflow and untouched(), change
    # as if it had not been called: the counter, the 32 newest frames, the ids and the place of what follows
    assert bytes(newest(L)) == before and int(newest(L).frame_id) == 62
    assert lib.get_last_frames(acq.bp, 32).tobytes() == newest_frames.tobytes()
    assert np.array_equal(lib.copy_frame(31).view(np.uint32), out[0].view(np.uint32))
    # a call on the 14 newest frames wraps to offset 0, clear of its sources
    first, _ = last.call()
    n = last.outputs
    assert first == 63 and int(lib.frame_info(63).device_pointer) == base and int(newest(L).device_pointer) == base + (n - 1) * each
    again = last.judge(lib.get_last_frames(acq.bp, n).copy(), newest_frames[18:])
    assert lib.get_last_frames(acq.bp, 14 + n)[:14].tobytes() == newest_frames[18:].tobytes()    # the sources, untouched
    print(f"refused: {len(refusals)} calls of {op.name} over their own 32 sources in a ring of {ring}; wrapped twice, {again:.4f} of the bound")


if __name__ == "__main__":
    main(sys.argv[1])
