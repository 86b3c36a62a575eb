"""Child process of tests/test_gpu_autocorr.py: beamformer_hip_autocorrelate_last_frames in a frame ring of
BEAMFORMER_HIP_FRAME_RING_BYTES = 1 MiB (the ring is sized once per process): 32 complex 64 x 1 x 64 frames of 32 KiB.  A run of lags is
at most four frames, so it meets its own sources only by wrapping: a burst of 16 and a mix 16 -> 15 leave 32 KiB at the end of the ring,
and the two lags of those 15 wrap to offset 0, clear of their sources; another burst of 16 and a mix 16 -> 14 then fill the ring to its
last byte, and one lag of the 32 newest frames -- the two lag frames at offset 0 among them -- would wrap onto the oldest of its own
sources: FrameSizeOverflow, and nothing has changed.
Started as python -m tests.autocorr_wrap_worker from the repository root (tests/scaffold.py run_ring_worker)."""
import ctypes as C
import os

import numpy as np

from ogl_beamforming_amd import configs as cfg, lib, params as P
from tests import autocorr_ref as ref
from tests import variants_cases as vc
from tests.frame_info import newest_info as newest


def share_of_bound(out, frames, W, lags):
    """the worst error of the lags as a share of its bound (lag 0's imaginary part must be 0 exactly)"""
    expected, bound = ref.autocorrelate(list(frames), W, lags)
    assert not out[0].imag.any()
    over = np.maximum(np.abs(out.real - expected.real), np.abs(out.imag - expected.imag))
    return float((over / np.maximum(bound, 1e-300)).max())


def main():
    ring = int(os.environ["BEAMFORMER_HIP_FRAME_RING_BYTES"])
    assert ring == 1 << 20
    L = lib.library()
    L.beamformer_set_global_timeout(0xFFFFFFFF)
    acq = cfg.rca("autocorr_wrap", 16, 2, 256, (64, 1, 64), vc.LO, vc.HI, seed=8950, interp=P.InterpolationMode.Linear, demodulate=False,
                  data_kind=P.DataKind.Float32Complex, angles=np.array([-6.0, 6.0]), kind=P.AcquisitionKind.RCA_TPW)
    rng = np.random.default_rng(8951)
    rf = rng.normal(0.0, 1.0, (16,) + acq.rf.shape).astype(acq.rf.dtype)
    W = (rng.standard_normal((16, 16)) + 1j * rng.standard_normal((16, 16))).astype(np.complex64)
    burst = lib.beamform_burst(acq.bp, rf, acq.filters).copy()                 # ids 0 .. 15 at offset 0 .. 512 KiB
    last = newest(L)
    each = int(last.size_bytes)
    base = int(last.device_pointer) - 15 * each
    assert each == 64 * 64 * 8 and int(last.frame_id) == 15 and 32 * each == ring

    # 16 -> 15: ids 16 .. 30 up to 992 KiB; their two lags (64 KiB) do not fit behind them: the run wraps to offset 0
    first, _ = lib.mix_last_frames(16, W[:15])
    mixed = lib.get_last_frames(acq.bp, 15).copy()
    assert first == 16 and int(newest(L).device_pointer) == base + 30 * each
    first, _ = lib.autocorrelate_last_frames(15, W[:15, :15], 2)
    lags = lib.get_last_frames(acq.bp, 2).copy()
    assert first == 31 and int(lib.frame_info(31).device_pointer) == base and int(newest(L).device_pointer) == base + each
    wrapped = share_of_bound(lags, mixed, W[:15, :15], 2)
    print(f"wrapped: two lags at offset 0, worst error {wrapped:.4f} of its bound")
    assert wrapped <= 1.0
    assert np.array_equal(lib.copy_frame(16).view(np.uint32), mixed[0].view(np.uint32))         # a source of the run
    assert np.array_equal(lib.copy_frame(2).view(np.uint32), burst[2].view(np.uint32))          # the burst behind the run is still there
    for gone in (0, 1):
        raw = np.zeros(each // 4, np.float32)
        assert not L.beamformer_hip_copy_frame(gone, raw.ctypes.data_as(C.c_void_p), raw.nbytes) and lib.last_error()[0] == P.LibError.InvalidAccess
        assert not L.beamformer_hip_get_frame_info(gone, C.byref(P.HipFrameInfo()))

    # a burst (ids 33 .. 48, 64 .. 576 KiB) and a mix 16 -> 14 (ids 49 .. 62) fill the ring to its last byte
    lib.beamform_burst(acq.bp, rf, acq.filters)
    first, _ = lib.mix_last_frames(16, W[:14])
    assert first == 49 and int(newest(L).device_pointer) == base + 31 * each and int(newest(L).frame_id) == 62
    # one lag of the 32 newest frames, ids 31 .. 62: 32 KiB do not fit behind them, and at offset 0 lies id 31 -- one of the call's sources
    newest_frames = lib.get_last_frames(acq.bp, 32).copy()
    out_id, ms = C.c_uint32(77), C.c_float(-1.0)
    before = bytes(newest(L))
    for pointer, rows in ((None, 32), (np.ones((1, 32), np.complex64).ctypes.data_as(C.POINTER(C.c_float)), 1)):
        assert not L.beamformer_hip_autocorrelate_last_frames(32, pointer, rows, 1, 0, C.byref(out_id), C.byref(ms))
        assert lib.last_error()[0] == P.LibError.FrameSizeOverflow and out_id.value == 77 and ms.value == -1.0
    # as if it had not been called: the counter, the 32 newest frames, the ids and the place of what follows
    assert bytes(newest(L)) == before and int(newest(L).frame_id) == 62
    assert lib.get_last_frames(acq.bp, 32).tobytes() == newest_frames.tobytes()
    assert np.array_equal(lib.copy_frame(31).view(np.uint32), lags[0].view(np.uint32))
    # four lags of the 14 newest frames wrap to offset 0, clear of their sources
    first, _ = lib.autocorrelate_last_frames(14, None, 4)
    assert first == 63 and int(lib.frame_info(63).device_pointer) == base and int(newest(L).device_pointer) == base + 3 * each
    again = share_of_bound(lib.get_last_frames(acq.bp, 4).copy(), newest_frames[18:], None, 4)
    assert again <= 1.0
    print(f"refused: a lag frame of {each} bytes over the oldest of its own 32 sources in a ring of {ring}; wrapped twice, {again:.4f} of the bound")


if __name__ == "__main__":
    main()
