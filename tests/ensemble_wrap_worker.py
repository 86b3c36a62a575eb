"""Child process of tests/test_gpu_ensemble.py: beamformer_hip_mix_last_frames in a frame ring of BEAMFORMER_HIP_FRAME_RING_BYTES =
1 MiB (the ring is sized once per process).  A burst of 16 complex 64 x 1 x 64 frames takes 512 KiB.  A mix 16 -> 16 fills the ring
exactly; the next one wraps to offset 0 and the burst's records stop being exportable; a mix 16 -> 17 would wrap onto its own sources:
FrameSizeOverflow, and nothing has changed.
Started as python -m tests.ensemble_wrap_worker from the repository root (tests/scaffold.py run_ring_worker)."""
import ctypes as C
import os

import numpy as np

from ogl_beamforming_amd import configs as cfg, lib, params as P
from tests import ensemble_ref as ref
from tests import variants_cases as vc
from tests.frame_info import newest_info as newest


def within_bound(out, frames, W):
    expected, bound = ref.mix(list(frames), W)
    over = np.maximum(np.abs(out.real - expected.real), np.abs(out.imag - expected.imag))
    return bool((over <= bound).all())


def main():
    ring = int(os.environ["BEAMFORMER_HIP_FRAME_RING_BYTES"])
    assert ring == 1 << 20
    L = lib.library()
    L.beamformer_set_global_timeout(0xFFFFFFFF)
    acq = cfg.rca("ensemble_wrap", 16, 2, 256, (64, 1, 64), vc.LO, vc.HI, seed=7950, interp=P.InterpolationMode.Linear, demodulate=False,
                  data_kind=P.DataKind.Float32Complex, angles=np.array([-6.0, 6.0]), kind=P.AcquisitionKind.RCA_TPW)
    rng = np.random.default_rng(7951)
    rf = rng.normal(0.0, 1.0, (16,) + acq.rf.shape).astype(acq.rf.dtype)
    W = (rng.standard_normal((16, 16)) + 1j * rng.standard_normal((16, 16))).astype(np.complex64)
    burst = lib.beamform_burst(acq.bp, rf, acq.filters).copy()                 # the ring's first frames: offset 0 .. 512 KiB
    last = newest(L)
    each = int(last.size_bytes)
    base = int(last.device_pointer) - 15 * each
    assert each == 64 * 64 * 8 and int(last.frame_id) == 15 and 32 * each == ring

    # 16 -> 16: fills the ring exactly
    first, _ = lib.mix_last_frames(16, W)
    a = lib.get_last_frames(acq.bp, 16).copy()
    assert first == 16 and int(newest(L).device_pointer) == base + 31 * each and int(lib.frame_info(16).device_pointer) == base + 16 * each
    assert within_bound(a, burst, W)
    assert np.array_equal(lib.copy_frame(0).view(np.uint32), burst[0].view(np.uint32))          # the burst is still there
    assert lib.last_burst_info().first_frame_id == 0

    # 16 -> 16 again: the run wraps to offset 0, over the burst, clear of its sources (the first run)
    first, _ = lib.mix_last_frames(16, W)
    b = lib.get_last_frames(acq.bp, 16).copy()
    assert first == 32 and int(lib.frame_info(32).device_pointer) == base and int(newest(L).device_pointer) == base + 15 * each
    assert within_bound(b, a, W)
    assert np.array_equal(lib.copy_frame(16).view(np.uint32), a[0].view(np.uint32))             # a source of the second run
    for gone in (0, 7, 15):
        raw = np.zeros(each // 4, np.float32)
        assert not L.beamformer_hip_copy_frame(gone, raw.ctypes.data_as(C.c_void_p), raw.nbytes) and lib.last_error()[0] == P.LibError.InvalidAccess
        assert not L.beamformer_hip_get_frame_info(gone, C.byref(P.HipFrameInfo()))

    # 16 -> 17: 544 KiB do not fit behind the second run, and at offset 0 they would overlap it -- the call's own sources
    W17 = np.concatenate([W, W[:1]])
    out_id, ms = C.c_uint32(77), C.c_float(-1.0)
    before = bytes(newest(L))
    assert not L.beamformer_hip_mix_last_frames(16, W17.ctypes.data_as(C.POINTER(C.c_float)), 17, 0, C.byref(out_id), C.byref(ms))
    assert lib.last_error()[0] == P.LibError.FrameSizeOverflow and out_id.value == 77 and ms.value == -1.0
    # as if it had not been called: the counter, the 16 newest frames, the ids and the place of what follows
    assert bytes(newest(L)) == before and int(newest(L).frame_id) == 47
    assert lib.get_last_frames(acq.bp, 16).tobytes() == b.tobytes()
    assert np.array_equal(lib.copy_frame(16).view(np.uint32), a[0].view(np.uint32))
    # a run the ring cannot hold at all
    W33 = np.concatenate([W, W, W[:1]])
    assert not L.beamformer_hip_mix_last_frames(16, W33.ctypes.data_as(C.POINTER(C.c_float)), 33, 0, C.byref(out_id), None)
    assert lib.last_error()[0] == P.LibError.FrameSizeOverflow and int(newest(L).frame_id) == 47
    # 16 -> 15 fits behind the second run
    first, _ = lib.mix_last_frames(16, W[:15])
    assert first == 48 and int(lib.frame_info(48).device_pointer) == base + 16 * each
    single = lib.beamform(acq.bp, rf[0], acq.filters)
    assert int(newest(L).frame_id) == 63 and int(newest(L).device_pointer) == base + 31 * each
    assert single.shape == burst[0].shape and np.isfinite(single.real).all()
    print(f"refused: a run of 17 frames of {each} bytes over its own sources in a ring of {ring}; wrapped once")


if __name__ == "__main__":
    main()
